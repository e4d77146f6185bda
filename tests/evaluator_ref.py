"""Torch fp32 restatement of the FGD evaluator's encoder (VAESKConv.map2latent = LocalEncoder, models/motion_encoder.py:698-787 over
models/utils/skeleton.py's SkeletonResidual): the yardstick of the HIP path for shapes tests/golden/evaluator_outputs.npz does not hold.
Pinned to that golden on CPU (tests/test_evaluator_host.py); runs on any device."""
import torch
import torch.nn.functional as F


def encode(sd: dict, x: torch.Tensor, layers: int = 4) -> torch.Tensor:
    """sd: a VAESKConv state_dict; x (B, n, 330) -> (B, n / 16, 240)."""
    h = x.float().permute(0, 2, 1)
    for i in range(layers):
        p = f"encoder.layers.{i}.0."
        r = F.conv1d(F.pad(h, (1, 1)), sd[p + "residual.0.weight"] * sd[p + "residual.0.mask"], sd[p + "residual.0.bias"], stride=2)
        r = F.group_norm(r, 10, sd[p + "residual.1.weight"], sd[p + "residual.1.bias"], 1e-5)
        s = F.conv1d(h, sd[p + "shortcut.weight"] * sd[p + "shortcut.mask"], sd[p + "shortcut.bias"], stride=2)
        o = r + s
        if p + "common.0.weight" in sd:
            o = torch.matmul(sd[p + "common.0.weight"], o)
        h = torch.tanh(o)
    return h.permute(0, 2, 1)
