"""The window-attention reference the SwinIR GPU tests share (tests/test_swinir_gpu.py,
tests/test_window_attention_edges_gpu.py): WindowAttention on natural-order tokens by the published network's own
steps, through oracle/swinir_path.py's window_partition, shift_mask and relative_position_index. It computes in the
dtype of its inputs: float64 is the reference, float32 the yardstick of what float32 arithmetic can reach."""
import torch

from oracle import swinir_path as sp


def attention_logits(qkv, table, B, H, W, heads, shift):
    """(scaled, biased, masked logits (B * nW, heads, 64, 64) in window-partition order, v (B * nW, heads, 64, hd))
    of the rolled and partitioned tokens."""
    C = qkv.shape[1] // 3
    x = qkv.view(B, H, W, 3 * C)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = sp.window_partition(x, 8).view(-1, 64, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = xw[0] * (C // heads) ** -0.5, xw[1], xw[2]
    attn = q @ k.transpose(-2, -1)
    idx = sp.relative_position_index(8)
    attn = attn + table[idx.view(-1)].view(64, 64, -1).permute(2, 0, 1).unsqueeze(0)
    if shift:
        mask = sp.shift_mask(H, W, 8, shift).to(attn.dtype)
        nW = mask.shape[0]
        attn = (attn.view(-1, nW, heads, 64, 64) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, 64, 64)
    return attn, v


def _attention_reference(qkv, table, B, H, W, heads, shift, rnd=None):
    """WindowAttention on natural-order tokens by the reference's own steps: roll, window_partition, bias lookup,
    mask, softmax, window_reverse, roll back (float64 for float64 inputs). rnd, when given, is applied to the
    probabilities and to the result (the two places where the bf16 kernel rounds)."""
    C = qkv.shape[1] // 3
    attn, v = attention_logits(qkv, table, B, H, W, heads, shift)
    p = attn.softmax(-1)
    if rnd is not None:
        p = rnd(p)
    out = (p @ v).transpose(1, 2).reshape(-1, 8, 8, C)
    out = sp.window_reverse(out, 8, H, W)
    if shift:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    out = out.reshape(B * H * W, C)
    return out if rnd is None else rnd(out)
