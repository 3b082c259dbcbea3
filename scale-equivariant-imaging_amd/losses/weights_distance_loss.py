"""Distance of a model's weights to those it started from (reference: src/losses/weights_distance_loss.py, added to
the training loss by demo/train.py:245-264 under --fine_tuning --weights_distance_loss):

    lambd * sum_k mean((p0_k - p_k)^2) / K        over the K named parameters, p0 = the weights at construction

A plain torch restatement: what `train.py --no-fused_optimizer` adds to the loss before backward(), and the comparand of
optim.FlatSGD, whose kernel folds the same penalty and its gradient into the optimizer step.
"""
import torch


class WeightsDistanceLoss:
    def __init__(self, pretrained_model, lambd, device):
        self.pretrained_weights = {name: p.detach().clone() for name, p in pretrained_model.named_parameters()}
        self.lambd = lambd
        self.device = device

    def __call__(self, model):
        weights = dict(model.named_parameters())
        if set(weights) != set(self.pretrained_weights):
            raise ValueError("the model's parameter names differ from those of the pretrained model")
        total = torch.zeros((), device=self.device)
        for name, anchor in self.pretrained_weights.items():
            total = total + torch.mean((anchor - weights[name]) ** 2)
        return self.lambd * total / len(self.pretrained_weights)
