"""fp64 references, error measures and input generators for the plan-free scalar kernels (loss buffer, Adam, uncertainties,
validation / training epilogue, evidential head): tests/test_scalar_reference_cpu.py checks the references against the host
classes, tests/test_scalar_kernels_gpu.py runs the kernels against them.

Every reference is dtype-generic: run on fp32 tensors it is "the reference in fp32 torch on the CPU", run on the same values
in fp64 it is the truth.  The distance between the two (yardstick) is the reference's own rounding on that input; a kernel
passes when its per-element error stays within MARGIN x that distance, never below MARGIN fp32 ulp.  Scalars handed to a
kernel through the C ABI are floats, so the references take them rounded to fp32 (f32): 0.999f is the beta2 the kernel was
given, not a rounding error of its own."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mimo_oracle as O
from tests.helpers import fp32_acc_bound, report

ULP32 = 2.0 ** -23
MARGIN = 4.0        # an equally long chain of fp32 operations in another order; device expf / logf at 1-2 ulp
COND_MARGIN = 8.0   # about eight fp32 roundings between a logit and a result
# floors, as fractions of a tensor's largest |reference| entry (elem_err compares |error| with max(|reference|, floor)):
FLOOR_SIGNED = 1e-3    # sums of signed O(1) inputs (means, error maps, NLL terms): their rounding error is absolute, ulp x the
                       # inputs' size; an entry 1000 x below the largest one is cancellation, not kernel arithmetic
FLOOR_POSITIVE = 1e-6  # gradients and sums of positive terms
TINY = 1e-30           # products and quotients of positive numbers: meaningful at every magnitude fp32 holds


def f32(x):
    """the value a C float argument carries"""
    return float(np.float32(x))


def to64(x):
    return x.double() if isinstance(x, torch.Tensor) and x.is_floating_point() else x


def frac_floor(frac):
    return lambda ref: max(frac * float(ref.abs().max()), 1e-300)


def elem_err(got, ref64, floor, where=None):
    """max over elements of |got - ref| / max(|ref|, floor) and the index of the worst element.  `floor`: a number or a
    tensor broadcastable to ref; `where`: only these elements.  A NaN / inf in `got` counts as an infinite error."""
    ref = torch.as_tensor(ref64, dtype=torch.float64).cpu()
    got = torch.as_tensor(got).detach().cpu().to(torch.float64).reshape(ref.shape)
    assert bool(torch.isfinite(ref).all()), "the fp64 reference must be finite for every element"
    fl = torch.as_tensor(floor, dtype=torch.float64)
    e = (got - ref).abs() / torch.maximum(ref.abs(), fl)
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, float("inf")))
    if where is not None:
        e = torch.where(where, e, torch.zeros_like(e))
    if e.numel() == 0:
        return 0.0, ()
    i = int(e.argmax())
    return float(e.flatten()[i]), tuple(int(k) for k in np.unravel_index(i, tuple(e.shape))) if e.dim() else ()


def _floor_of(floors, k, ref):
    fl = floors[k]
    return fl(ref) if callable(fl) else fl


def yardstick(fn, inputs, floors, fn64=None):
    """How far `fn` in fp32 torch on the CPU sits from `fn` (or `fn64`) in fp64 on the same fp32 inputs, per output quantity
    (fn returns {name: tensor}), measured with elem_err over the elements where the fp32 result is finite.  Returns
    ({name: error}, the fp64 results, {name: mask of elements whose fp32 result is NOT finite})."""
    lo = fn(*inputs)
    hi = (fn64 or fn)(*[to64(x) for x in inputs])
    errs, bad = {}, {}
    for k, ref in hi.items():
        fin = torch.isfinite(lo[k].double())
        bad[k] = ~fin
        errs[k] = elem_err(torch.where(fin, lo[k].double(), ref), ref, _floor_of(floors, k, ref))[0]
    return errs, hi, bad


def bound(y):
    """per-element bound from a yardstick: MARGIN x it, never below MARGIN fp32 ulp"""
    return MARGIN * max(y, ULP32)


def check(kernel, name, got, ref64, floor, y, where=None):
    """elem_err(got, ref64) <= bound(y); reports error, yardstick, and their ratio (error / max(yardstick, 1 ulp))."""
    e, at = elem_err(got, ref64, floor, where)
    ratio = e / max(y, ULP32)
    report(f"[{kernel}] {name}: err {e:.2e} yardstick {y:.2e} ratio {ratio:.2f} worst at {at}")
    assert e <= bound(y), (kernel, name, e, y, at)
    return ratio


def conditioning(fn64, inputs, arg, channel_dim=1):
    """Conditioning of fn64's results under fp32 rounding of input `arg` (a [N, C, ...] tensor of fp32 values): each channel
    moved one fp32 ulp up and one down (torch.nextafter) with the others in place, fn64 re-evaluated in fp64; per output
    element the largest |change| over the 2 C moves.  (fn64 is pixel-local, so all pixels move at once.)"""
    x32 = inputs[arg].float()
    base = fn64(*[to64(x) for x in inputs])
    worst = {k: torch.zeros_like(v) for k, v in base.items()}
    for c in range(x32.shape[channel_dim]):
        for toward in (float("inf"), -float("inf")):
            moved = x32.clone()
            sel = moved.select(channel_dim, c)
            sel.copy_(torch.nextafter(sel, torch.full_like(sel, toward)))
            args = [to64(moved if i == arg else x) for i, x in enumerate(inputs)]
            for k, v in fn64(*args).items():
                worst[k] = torch.maximum(worst[k], (v - base[k]).abs())
    return worst


def check_conditioned(kernel, name, got, ref64, floor, cond, where):
    """Elements `where` the fp32 reference is not finite: |got - ref| <= max(COND_MARGIN x cond, MARGIN ulp of max(|ref|,
    floor)) per element.  Reports the worst error / conditioning ratio."""
    ref = ref64.double()
    got = torch.as_tensor(got).detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(ref).all())
    if not bool(where.any()):
        return 0.0
    fl = torch.as_tensor(floor, dtype=torch.float64)
    allowed = torch.maximum(COND_MARGIN * cond, MARGIN * ULP32 * torch.maximum(ref.abs(), fl))
    err = torch.where(torch.isfinite(got), (got - ref).abs(), torch.full_like(ref, float("inf")))
    q = torch.where(where, err / (allowed / COND_MARGIN), torch.zeros_like(err))  # in units of the conditioning yardstick
    i = int(q.argmax())
    at = tuple(int(k) for k in np.unravel_index(i, tuple(q.shape)))
    report(f"[{kernel}] {name} (fp32 reference not finite, {int(where.sum())} elements): worst err / conditioning "
           f"{float(q.flatten()[i]):.2f} (margin {COND_MARGIN:g}) at {at}: got {float(got.flatten()[i]):.9e} ref {float(ref.flatten()[i]):.9e}")
    assert float(q.flatten()[i]) <= COND_MARGIN, (kernel, name, float(q.flatten()[i]), at)
    return float(q.flatten()[i])


def check_scalar(kernel, name, got, ref, y_terms, term_scale):
    """A reduced scalar accumulated in double from fp32 per-element terms: |got - ref| <= MARGIN x (yardstick of the terms) x
    (mean of max(|term|, floor) = term_scale) + the final conversion to float (fp32_acc_bound(1, 0) = 2^-24 of |ref|)."""
    allowed = bound(y_terms) * term_scale + fp32_acc_bound(1, 0.0) * abs(ref)
    e = abs(float(got) - float(ref))
    report(f"[{kernel}] scalar {name}: got {float(got):.9e} ref {float(ref):.9e} err {e:.2e} allowed {allowed:.2e} "
           f"ratio {e / max(allowed / MARGIN, 1e-300):.2f}")
    assert e <= allowed, (kernel, name, float(got), float(ref), allowed)
    return e / max(allowed / MARGIN, 1e-300)


# ---- loss buffer -------------------------------------------------------------------------------------------------------

LOSS_BUFFER_S = (1, 2, 3, 63, 64)
LOSS_BUFFER_SIZES = (1, 10)
LOSS_BUFFER_T = (0.3, 0.01)
LOSS_BUFFER_STEPS = 25


def loss_buffer_losses(S, size, T, steps=LOSS_BUFFER_STEPS):
    """[steps, S] fp32 losses drawn from [-5, 40]: mean / T spans thousands at T = 0.01"""
    g = torch.Generator().manual_seed(1000 * S + 10 * size + int(T * 100))
    return torch.rand(steps, S, generator=g) * 45.0 - 5.0


def loss_buffer_sequence(losses, S, T, size):
    """O.LossBuffer over the rows of `losses` in the losses' dtype: per step the weights (read BEFORE the loss is added),
    weights / S, mean(loss * weights), mean(loss) and the ring after the step."""
    lb = O.LossBuffer(S, f32(T), size)
    lb.buffer = lb.buffer.to(losses.dtype)
    out = {"weights": [], "w_over_s": [], "weighted": [], "mean": [], "ring": []}
    for l in losses:
        w = lb.get_weights()
        lb.add(l)
        out["weights"].append(w)
        out["w_over_s"].append(w / S)
        out["weighted"].append((l * w).mean())
        out["mean"].append(l.mean())
        out["ring"].append(lb.buffer.clone())
    return {k: torch.stack(v) for k, v in out.items()}


def loss_buffer_floors(losses):
    # weights sum to S: below 1e-6 a weight moves the weighted mean by less than an ulp of it; the two scalars are sums of
    # signed losses of size max |loss|
    lmax = float(losses.abs().max())
    return {"weights": FLOOR_POSITIVE, "w_over_s": FLOOR_POSITIVE / losses.shape[1], "weighted": FLOOR_SIGNED * lmax,
            "mean": FLOOR_SIGNED * lmax, "ring": TINY}


# ---- Adam --------------------------------------------------------------------------------------------------------------

ADAM_SIZES = (1, 3, 4, 5, 2097152 + 7)
ADAM_HYPER = [(wd, gs, step) for wd in (0.0, 1e-2) for gs in (1.0, 1.0 / 3.0) for step in (1, 2, 100000)]
ADAM_HYPER_LARGE = [(0.0, 1.0, 1), (1e-2, 1.0 / 3.0, 2), (1e-2, 1.0, 100000), (0.0, 1.0 / 3.0, 100000)]


def adam_inputs(n, step):
    """p, g, m, v (fp32).  The moments are those `step - 1` earlier steps leave: zero before the first, beta-weighted sums of
    gradients of g's size after.  m carries g's sign, so beta1 m + (1 - beta1) g does not cancel and the per-element
    relative error measures the kernel's roundings, not the conditioning of that sum."""
    gen = torch.Generator().manual_seed(n % 1000 + step)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen)
    if step == 1:
        return p, g, torch.zeros(n), torch.zeros(n)
    k = 1.0 - 0.9 ** (step - 1)
    m = torch.sign(g) * torch.rand(n, generator=gen) * k
    v = (torch.rand(n, generator=gen) + 0.05) * (1.0 - 0.999 ** (step - 1))
    return p, g, m, v


def adam_reference(p, g, m, v, *, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, grad_scale=1.0):
    """O.adam_update on g * grad_scale in the tensors' dtype, hyperparameters as the floats the C ABI carries"""
    p, m, v = p.clone(), m.clone(), v.clone()
    O.adam_update(p, g * f32(grad_scale), m, v, step, f32(lr), f32(beta1), f32(beta2), f32(eps), f32(wd))
    return {"p": p, "m": m, "v": v}


def adam_floors(p, ref):
    # a parameter is meaningful down to one update: the largest |p' - p| of the tensor (its own rounding is an ulp of |p'|,
    # the update's an ulp of the update)
    return {"p": max(float((ref["p"] - p.double()).abs().max()), 1e-300), "m": frac_floor(FLOOR_POSITIVE),
            "v": frac_floor(FLOOR_POSITIVE)}


# ---- uncertainties and the two epilogues ------------------------------------------------------------------------------------

EPS_MIN, EPS_MAX = O.EPS_MIN, O.EPS_MAX
CLAMP_EDGES = (-20.0, float(np.log(np.float32(EPS_MIN))), float(np.log(np.float32(EPS_MAX))), 9.0)


def plant_clamp_edges(log_param):
    """log-dispersion planes [..., hw]: -20, ln eps_min, ln eps_max and +9 in the first and in the last elements"""
    flat = log_param.reshape(-1)
    for i, val in enumerate(CLAMP_EDGES):
        flat[i] = val
        flat[-1 - i] = val
    return log_param


def uncertainty_inputs(N, S, C, hw, seed):
    g = torch.Generator().manual_seed(seed)
    p1 = torch.randn(N, S, C, 1, hw, generator=g)
    p2 = plant_clamp_edges(torch.randn(N, S, C, 1, hw, generator=g))
    return p1, p2


def uncertainties_reference(kind):
    def fn(p1, p2):
        mean, alea, epi = O.compute_uncertainties(kind, p1, p2)
        return {"mean": mean, "aleatoric_var": alea, "epistemic_var": epi}
    return fn


# variances: the loss clamps the dispersion at eps_min, nothing below its square is meaningful; the epistemic variance and the
# mean are formed from sums / differences of the signed predictions
UNCERTAINTY_FLOORS = {"mean": frac_floor(FLOOR_SIGNED), "aleatoric_var": EPS_MIN ** 2, "epistemic_var": frac_floor(FLOOR_SIGNED)}


def validation_inputs(N, S, Ct, hw, seed, zero_images=(0,)):
    """logits [N,S,2Ct,1,hw] with the clamp edges planted, label [N,Ct,1,hw], mask [N,1,1,hw] with the images `zero_images`
    wholly zero and 30 % zeros elsewhere"""
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(N, S, 2 * Ct, 1, hw, generator=g)
    plant_clamp_edges(out[0, 0, Ct])
    plant_clamp_edges(out[N - 1, S - 1, 2 * Ct - 1])
    label = torch.randn(N, Ct, 1, hw, generator=g)
    mask = (torch.rand(N, 1, 1, hw, generator=g) > 0.3).float()
    for n in zero_images:
        if N > 1:
            mask[n] = 0.0
    return out, label, mask


def validation_reference(kind):
    """the tail of validation_step (mimo_unet.py:153-183) from the oracle's operators: the four maps and the per-element terms
    of the reduced scalars"""
    def fn(out, label, mask):
        Ct = out.shape[2] // 2
        p1, p2 = out[:, :, :Ct], out[:, :, Ct:]
        mean, alea, epi = O.compute_uncertainties(kind, p1, p2)
        comb = O.calculate_dist_param(kind, torch.sqrt(alea + epi), log=True)
        nll = O.loss_forward(kind, p1.mean(dim=1), comb, label, mask=mask, reduce_mean=False)
        a_std, e_std, err = alea.sqrt(), epi.sqrt(), mean - label
        return {"mean": mean, "aleatoric_std": a_std, "epistemic_std": e_std, "err": err, "nll": nll, "abs_err": err.abs(),
                "sq_err": err * err, "aleatoric_clip": a_std.clip(0, 5), "epistemic_clip": e_std.clip(0, 5)}
    return fn


VALIDATION_FLOORS = {"mean": frac_floor(FLOOR_SIGNED), "aleatoric_std": EPS_MIN, "epistemic_std": frac_floor(FLOOR_SIGNED),
                     "err": frac_floor(FLOOR_SIGNED), "nll": frac_floor(FLOOR_SIGNED), "abs_err": frac_floor(FLOOR_SIGNED),
                     "sq_err": frac_floor(FLOOR_SIGNED), "aleatoric_clip": EPS_MIN, "epistemic_clip": frac_floor(FLOOR_SIGNED)}


def regression_scalars(terms, label):
    """metrics.py:22-34 in fp64 from the fp64 terms"""
    y = label.double().flatten()
    sse, ss_tot = terms["sq_err"].sum(), ((y - y.mean()) ** 2).sum()
    mse = terms["sq_err"].mean()
    return {"mae": float(terms["abs_err"].mean()), "mse": float(mse), "rmse": float(mse.sqrt()), "r2": float(1 - sse / ss_tot),
            "sse_over_ss_tot": float(sse / ss_tot), "count": float(terms["sq_err"].numel())}


def term_scale(ref, floor):
    """mean of max(|term|, floor): what a per-element relative error of the terms is relative to in their mean"""
    return float(torch.maximum(ref.abs(), torch.as_tensor(floor, dtype=torch.float64)).mean())


def training_inputs(N0, reps, S, Ct, hw, seed):
    g = torch.Generator().manual_seed(seed)
    N = N0 * reps
    out = torch.randn(N, S, 2 * Ct, 1, hw, generator=g)
    plant_clamp_edges(out[0, 0, Ct])
    plant_clamp_edges(out[N - 1, S - 1, 2 * Ct - 1])
    label = torch.randn(N0, Ct, 1, hw, generator=g)
    perms = O.draw_perms(N0, S, 0.0, reps, generator=g)
    return out, label, perms


def training_reference(kind):
    def fn(out, label, perms):
        Ct, S = out.shape[2] // 2, out.shape[1]
        p1, p2 = out[:, :, :Ct], out[:, :, Ct:]
        label_t = torch.stack([label[perms[s]] for s in range(S)], dim=1)
        err = p1 - label_t
        return {"label_t": label_t, "preds": p1, "aleatoric_std": O.loss_std(kind, p2), "err": err, "abs_err": err.abs(),
                "sq_err": err * err}
    return fn


TRAINING_FLOORS = {"label_t": TINY, "preds": TINY, "aleatoric_std": EPS_MIN, "err": frac_floor(FLOOR_SIGNED),
                   "abs_err": frac_floor(FLOOR_SIGNED), "sq_err": frac_floor(FLOOR_SIGNED)}


# ---- evidential head -----------------------------------------------------------------------------------------------------

def inverse_softplus(x):
    """fp64 logit whose softplus (threshold 20, as torch and the kernels take it) is x"""
    x = torch.as_tensor(x, dtype=torch.float64)
    return torch.where(x > 20, x, torch.log(torch.expm1(x.clamp(max=20.0))))


EVIDENTIAL_ALPHA_M1 = [10.0 ** (k / 2.0) for k in range(-8, 9)] + [19.5, 20.5]  # 1e-4 .. 1e4 and both sides of the threshold
EVIDENTIAL_V = [1e-3, 10.0 ** -1.5, 1.0, 10.0 ** 1.5, 1e3]
EVIDENTIAL_BETA = EVIDENTIAL_V
EVIDENTIAL_DIFF = [0.0, 1e-3, 1.0, 30.0]


def evidential_sweep():
    """One pixel per combination of alpha - 1, v, beta and |y - mu| (1900 pixels): logits [P, 4], label [P], mask [P] (every
    seventh pixel 0), all fp32, and the alpha - 1 of each pixel."""
    am1, v, b, d = (t.flatten() for t in torch.meshgrid(*[torch.tensor(x, dtype=torch.float64) for x in (
        EVIDENTIAL_ALPHA_M1, EVIDENTIAL_V, EVIDENTIAL_BETA, EVIDENTIAL_DIFF)], indexing="ij"))
    P = am1.numel()
    g = torch.Generator().manual_seed(35)
    mu = torch.randn(P, generator=g)
    sign = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0)
    logits = torch.stack([mu, inverse_softplus(v).float(), inverse_softplus(am1).float(), inverse_softplus(b).float()], dim=1)
    label = (mu.double() + sign * d).float()
    mask = (torch.arange(P) % 7 != 3).float()
    return logits, label, mask, am1


def evidential_ordinary(P, seed=36):
    """P pixels of ordinary values: logits ~ N(0, 1) (alpha in (1, ~6)), labels within a few units of mu, 20 % masked"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(P, 4, generator=g)
    label = logits[:, 0] + torch.randn(P, generator=g)
    mask = (torch.rand(P, generator=g) > 0.2).float()
    return logits, label, mask


def pixels_to_layout(logits, label, mask, N):
    """[P, 4] / [P] pixel lists -> logits [N, 4, hw], label [N, hw], mask [N, hw]"""
    P = logits.shape[0]
    hw = P // N
    assert hw * N == P
    return logits.view(N, hw, 4).permute(0, 2, 1).contiguous(), label.view(N, hw).contiguous(), mask.view(N, hw).contiguous()


def nig_heads(logits):
    mu, lv, la, lb = torch.unbind(logits, dim=1)
    return torch.stack([mu, F.softplus(lv), F.softplus(la) + 1, F.softplus(lb)], dim=1)


def evidential_loss_lgamma_difference(ev, y, mask=None):
    """O.evidential_loss with G(alpha) = exp(lgamma(alpha - 1/2) - lgamma(alpha)) / 4: the same function, finite in fp64 for
    every alpha (the oracle's exp(lgamma) / exp(lgamma) is inf / inf from alpha = 172 on in fp64, from 35 on in fp32).  In
    fp64 the difference of the two lgammas is good to 1e-11 at alpha = 1e4."""
    mu, v, alpha, beta = torch.unbind(ev, dim=1)
    coeff = torch.exp(torch.lgamma(alpha - 0.5) - torch.lgamma(alpha)) / (4 * v * torch.sqrt(beta))
    loss = coeff * (2 * beta * (1 + v) + (2 * alpha - 1) * v * (y - mu) ** 2) + (y - mu) ** 2 * (2 * alpha + v)
    return loss * mask if mask is not None else loss


def evidential_reference(loss_form, up_loss=True, up_ev=True):
    """fn(logits [N,4,hw], label [N,hw], mask [N,hw], d_loss [N,hw], d_ev [N,4,hw]) -> NIG parameters, loss map, the two
    variances and dlogits of sum(loss * d_loss) + sum(ev * d_ev) by autograd (either upstream gradient can be left out)."""
    def fn(logits, label, mask, d_loss, d_ev):
        lt = logits.detach().clone().requires_grad_(True)
        ev = nig_heads(lt)
        loss = loss_form(ev, label, mask)
        total = lt.sum() * 0.0
        if up_loss:
            total = total + (loss * d_loss).sum()
        if up_ev:
            total = total + (ev * d_ev).sum()
        (dlogits,) = torch.autograd.grad(total, lt)
        alea, epi = O.evidential_vars(ev.detach())
        return {"ev": ev.detach(), "loss": loss.detach(), "dlogits": dlogits, "aleatoric_var": alea, "epistemic_var": epi}
    return fn


def evidential_oracle_form(ev, y, mask=None):
    """O.evidential_loss; NaN (value and gradient) where one of its two exponentiated lgammas or its denominator
    4 Gamma(alpha) v sqrt(beta) has overflowed the dtype: inf / inf is NaN by itself, finite / inf is a silent 0 that is no
    rounding of anything — both mean "the reference has no result in this dtype here"."""
    loss = O.evidential_loss(ev, y[:, None], mask)
    _, v, alpha, beta = torch.unbind(ev.detach(), dim=1)
    ok = torch.isfinite(torch.exp(torch.lgamma(alpha - 0.5))) & torch.isfinite(4 * torch.exp(torch.lgamma(alpha)) * v * torch.sqrt(beta))
    return loss * torch.where(ok, 1.0, float("nan")).to(loss.dtype)  # (a factor: its NaN reaches the gradient of these pixels only)


def evidential_floors(ref):
    # dlogits: the four components of a pixel feed one 1 x 1 head's backward; 1e-6 of the pixel's largest component
    g = ref["dlogits"]
    return {"ev": TINY, "loss": TINY, "aleatoric_var": TINY, "epistemic_var": TINY,
            "dlogits": (FLOOR_POSITIVE * g.abs().amax(dim=1, keepdim=True)).clamp_min(1e-300).expand_as(g)}
