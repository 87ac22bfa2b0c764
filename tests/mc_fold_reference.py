"""fp64 numpy model of `fold_image_grad_mc_kernel` (csrc/ew_layout.hip): the transpose of `reflect-pad -> repeat over
the passes`, shared by tests/test_mc_adversarial_cpu.py (which checks it against torch autograd) and
tests/test_mc_adversarial_gpu.py (which checks the kernel against it)."""
import numpy as np


def fold(dxpad):
    """dxpad [N,H+2,W+2,C] on the reflect-padded domain -> [N,H,W,C]: pad row -1 lands on row 1, pad row H on row H-2, the
    same for columns (corners take both steps)."""
    f = np.array(dxpad, dtype=np.float64)
    H, W = f.shape[1] - 2, f.shape[2] - 2
    assert H >= 2 and W >= 2
    f[:, 2] += f[:, 0]
    f[:, H - 1] += f[:, H + 1]
    f[:, :, 2] += f[:, :, 0]
    f[:, :, W - 1] += f[:, :, W + 1]
    return f[:, 1:H + 1, 1:W + 1]


def fold_mc(dxpad, replicas, channels, start=None):
    """dxpad [R*B,H+2,W+2,ldp], pass-major (pass m, image b at row m*B + b) -> dimage [B,channels,H,W] in fp64:
    start (or 0) + sum over the passes of the folded gradient's first `channels` channels."""
    n = dxpad.shape[0]
    assert replicas >= 1 and n % replicas == 0
    f = fold(dxpad)[..., :channels]
    f = f.reshape(replicas, n // replicas, *f.shape[1:]).sum(axis=0)
    out = np.ascontiguousarray(f.transpose(0, 3, 1, 2))
    return out if start is None else out + np.asarray(start, dtype=np.float64)
