"""The captured training step with the groupable fused-Adam weight gradients queued and issued as ONE grouped launch at
the end of the backward pass (models/_wgrad.py, ADAM_GROUP) against the same step with every launch where its gradient
arrives (SEI_NO_ADAM_GROUP=1), after one and two replays and after one eager step from the same start with the sinks
registered (bench.py's record_one_step). Each configuration is a fresh process (tests/adam_group_worker.py): the switch
is read when models/_wgrad.py is imported.

BIT FOR BIT: the losses; parameter, exp_avg and exp_avg_sq on the ranges of the flat buckets that the fused GEMMs own
(everything the grouped launch writes, 2,097,152 of the bucket's 2,567,104 elements here); the WHOLE bf16 shadow bucket.
The grouped launch runs every job's tiles through the kernel body of its own launch, and nothing between the two launch
positions reads or writes what it touches, so nothing there may differ.

The rest of the float32 buckets cannot be compared bit for bit between two processes: the weight gradients of the
shallow levels are summed with float atomics (streamed launch, split K), whose order differs from run to run. Measured
on one MI355X, six runs, every pair: two runs of the SAME configuration differ in 2,501 - 3,607 parameters, 134,724 -
200,663 exp_avg and 149,808 - 222,378 exp_avg_sq elements after one replay (5,688 - 7,943 / 155,979 - 212,341 /
176,254 - 239,975 after two), all of them outside the fused ranges, and grouped against ungrouped lies in the same
band; inside the fused ranges and in the shadow bucket no pair differed in any element. Outside the ranges the
parameters are therefore held to what `steps` Adam steps can move one element at all: each step moves it by at most
lr max(1, (1 - beta1) / sqrt(1 - beta2)), two runs can be that far apart in opposite directions.
"""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "adam_group_worker.py")
LR, BETA1, BETA2 = 3e-4, 0.9, 0.999            # the worker's FlatAdam
STEPS = {"after_replay_1": 1, "after_replay_2": 2, "after_eager": 1}


def _run(tmp_path, name, no_group):
    out = str(tmp_path / f"{name}.pt")
    env = dict(os.environ)
    env.pop("SEI_NO_ADAM_GROUP", None)
    if no_group:
        env["SEI_NO_ADAM_GROUP"] = "1"
    r = subprocess.run([sys.executable, WORKER, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("adam_group")
    return _run(tmp, "grouped", False), _run(tmp, "apart", True)


def test_the_deepest_level_is_registered_and_served(runs):
    for run in runs:
        assert run["shapes"] == [(512, 2048), (2048, 512)]                  # whole 128 x 256 tiles, one round each
        assert run["served"]                                                # fused_adam_launches == the registered views
        assert sum(hi - lo for lo, hi in run["fused_ranges"]) == 2 * 512 * 2048


def test_grouped_step_issues_one_launch_and_has_fewer_kernel_nodes(runs):
    grouped, apart = runs
    assert grouped["entries"] == ["sei_gemm_bf16nt_dw2_adam_group"] and grouped["group_jobs"] == [2]
    assert apart["entries"] == ["sei_gemm_bf16nt_dw2_adam"] * 2
    assert grouped["kernel_nodes"] == apart["kernel_nodes"] - 1


@pytest.mark.parametrize("when", sorted(STEPS))
def test_grouped_step_equals_separate_launches(runs, when):
    grouped, apart = runs
    assert grouped["losses"] == apart["losses"]
    assert grouped["fused_ranges"] == apart["fused_ranges"]
    inside = torch.zeros(grouped[when][0].numel(), dtype=torch.bool)
    for lo, hi in grouped["fused_ranges"]:
        inside[lo:hi] = True
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), grouped[when], apart[when]):
        differ = a != b
        print(f"{when} {name}: {int((differ & inside).sum())} elements differ inside the fused ranges, "
              f"{int((differ & ~inside).sum())} outside")
        assert not bool((differ & inside).any()), (when, name, int((differ & inside).sum()))
    assert torch.equal(grouped[when][3].view(torch.int16), apart[when][3].view(torch.int16)), (when, "bf16 shadow")
    reach = 2 * STEPS[when] * LR * max(1.0, (1 - BETA1) / (1 - BETA2) ** 0.5)
    assert float((grouped[when][0] - apart[when][0]).abs().max()) <= reach
    assert not torch.equal(grouped[when][0], grouped["after_replay_2" if when != "after_replay_2" else "after_replay_1"][0])
