"""Numpy restatement of the FGSM step (what `fgsm_attack` of the reference's scripts/test/test_nyuv2_depth.py:16-24
computes) and of the sign rule the adversarial tests share.  fp32 throughout, like the torch original."""
import numpy as np

# a pixel's sign is DECIDED when |g| >= DECIDED_REL * max|g|: DECIDED_REL is the project's output tolerance
# (max|a - b| / max|b| <= 1e-3), so a gradient that passes that tolerance cannot flip a decided pixel
DECIDED_REL = 1e-3
MAX_UNDECIDED_SHARE = 0.02  # condition on a test input (checked on the reference's own gradient), not a measurement


def fgsm_attack(image, epsilon, data_grad, lo=0.0, hi=1.0):
    """clamp(image + epsilon * sign(data_grad), lo, hi) in fp32; sign(0) = 0.  A NaN gradient gives a NaN pixel (np.sign
    propagates it; torch.sign would return 0 there) — the rule the engine's kernel follows."""
    image = np.asarray(image, dtype=np.float32)
    step = np.float32(epsilon) * np.sign(np.asarray(data_grad, dtype=np.float32))
    out = (image + step).astype(np.float32)
    clipped = np.minimum(np.maximum(out, np.float32(lo)), np.float32(hi))
    return np.where(np.isnan(out), out, clipped).astype(np.float32)


def decided(grad_ref):
    g = np.abs(np.asarray(grad_ref, dtype=np.float64))
    return g >= DECIDED_REL * g.max()


def undecided_share(grad_ref):
    return 1.0 - float(decided(grad_ref).mean())


def sum_over_subnetworks(dx):
    """[N,S,C,H,W] -> [N,C,H,W] in the engine's documented order: s = S-1 first, then S-2, ..., 0 (fp32 adds)."""
    dx = np.asarray(dx, dtype=np.float32)
    acc = dx[:, -1].copy()
    for s in range(dx.shape[1] - 2, -1, -1):
        acc = (acc + dx[:, s]).astype(np.float32)
    return acc
