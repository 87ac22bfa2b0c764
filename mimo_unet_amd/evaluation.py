"""`UncertaintyEvaluator`: the sparsification and calibration tables of the reference's test scripts
(``scripts/test/test_nyuv2_depth.py:93-170``, ``scripts/test/test_ndvi.py:52-128``), formed on the GPU.

The reference moves every pixel of the test set to the host, builds a pandas frame, sorts it by `combined_std` for
`precision_recall.csv` and sweeps 41 `scipy.stats.norm.ppf` calls over it for `calibration.csv`.  Here each batch is
reduced where `EnsembleModule(keep_on_device=True)` leaves it: one pass (`mimo_eval_accumulate`) appends an 8-byte
record per pixel to a device store and bumps the calibration counters; `compute()` selects the 100 cutoff keys exactly
with three counting passes (`mimo_eval_select`), sums the intervals between them (`mimo_eval_interval_sums`) and copies
one small buffer to the host.  No pandas, no scipy, no CPU path.

    ev = UncertaintyEvaluator()
    for batch in loader:
        ev.update_from(ensemble, batch["image"].cuda(), batch["label"].cuda())
    ev.write_csv(result_dir)

Opt-in, `sources=("combined", "aleatoric", "epistemic")`: the same sparsification curve per uncertainty source and the
oracle curve (pixels dropped by their own error), and their areas AUSE / AURG (`sparsification_areas`).  The pass then
writes a second 8-byte record per pixel (`mimo_eval_accumulate_sources`) and `compute()` runs the selection once per
ordering over the word that holds its key (`mimo_eval_select_by`, `mimo_eval_interval_sums_by`), still ending in one copy.
"""
from __future__ import annotations

import os
import warnings
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

MAX_PERCENTILES = 128  # eval_stats.hip: kMaxP
MAX_THRESHOLDS = 64    # eval_stats.hip: kMaxK
PRECISION_RECALL_HEADER = ("percentile", "mae", "rmse")       # test_nyuv2_depth.py:142
CALIBRATION_HEADER = ("Expected Conf.", "Observed Conf.")     # test_nyuv2_depth.py:169
# orderings of the sparsification curve -> (store, word) that holds the key; store 0 = records, 1 = source records
SOURCES = {"combined": (0, 0), "aleatoric": (1, 0), "epistemic": (1, 1), "oracle": (0, 1)}

_NDTRI_P0 = (-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1,
             -1.23916583867381258016E0)
_NDTRI_Q0 = (1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1, -2.25462687854119370527E2,
             2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1, -1.18331621121330003142E0)


def cutoff_indices(percentiles, n: int) -> np.ndarray:
    """How many of the most uncertain pixels each row drops: the truncation of the float64 product
    `(percentiles * N).astype(int)` (test_nyuv2_depth.py:137) — not integer arithmetic.  The evaluator itself forms
    these ranks on the device (eval_select_init_kernel: the pixel count never visits the host before the final copy),
    with this arithmetic; the function mirrors that kernel for callers (plots, checks) and for the tests."""
    p = np.asarray(percentiles, dtype=np.float64)
    return np.clip((p * np.float64(n)).astype(np.int64), 0, n)


def standard_quantiles(expected_p, distribution: str = "norm") -> np.ndarray:
    """z_k = ppf(p_k) of the standard distribution in float64; -inf at p = 0 and +inf at p = 1.  "norm" is what the
    reference passes for every model (test_nyuv2_depth.py:233); "laplace" is the closed form of scipy.stats.laplace."""
    p = np.asarray(expected_p, dtype=np.float64)
    if distribution == "norm":
        z = torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(p))).numpy()
        # Central region (exp(-2) < p < 1 - exp(-2)): Cephes' rational approximation (ndtri.c, the routine behind
        # scipy.special.ndtri) evaluated step by step in float64, so that the table does not depend on how a build of
        # torch contracts the same polynomial (2 ulp were seen); the tails stay torch's.
        mid = np.minimum(p, 1.0 - p) > 0.13533528323661269189
        y = p[mid] - 0.5
        y2 = y * y
        num, den = np.full_like(y2, _NDTRI_P0[0]), y2 + _NDTRI_Q0[0]
        for c in _NDTRI_P0[1:]:
            num = num * y2 + c
        for c in _NDTRI_Q0[1:]:
            den = den * y2 + c
        z[mid] = (y + y * (y2 * num / den)) * 2.50662827463100050242
        return z
    if distribution == "laplace":
        with np.errstate(divide="ignore"):
            return np.where(p > 0.5, -np.log(2.0 * (1.0 - p)), np.log(2.0 * p))
    raise ValueError(f"distribution must be 'norm' or 'laplace', not {distribution!r}")


def write_tables_csv(tables: dict, directory: str) -> Tuple[str, str]:
    """`precision_recall.csv` and `calibration.csv` with the reference's headers (what `DataFrame.to_csv(index=False)`
    writes, test_nyuv2_depth.py:229,234)."""
    os.makedirs(directory, exist_ok=True)
    pr, cal = tables["precision_recall"], tables["calibration"]
    paths = (os.path.join(directory, "precision_recall.csv"), os.path.join(directory, "calibration.csv"))
    with open(paths[0], "w") as f:
        f.write(",".join(PRECISION_RECALL_HEADER) + "\n")
        for row in zip(pr["percentile"], pr["mae"], pr["rmse"]):
            f.write(",".join(repr(float(v)) for v in row) + "\n")
    with open(paths[1], "w") as f:
        f.write(",".join(CALIBRATION_HEADER) + "\n")
        for row in zip(cal["expected"], cal["observed"]):
            f.write(",".join(repr(float(v)) for v in row) + "\n")
    return paths


def check_sources(sources) -> Tuple[str, ...]:
    """The requested orderings, in the order given, without repeats; an unknown name raises ValueError."""
    names = (sources,) if isinstance(sources, str) else tuple(sources)
    for name in names:
        if name not in SOURCES:
            raise ValueError(f"unknown uncertainty source {name!r}: choose from {tuple(SOURCES)}")
    return tuple(dict.fromkeys(names))


def sparsification_areas(percentiles, curve, oracle, normalize: bool = False) -> Tuple[float, float]:
    """(AUSE, AURG) of one sparsification curve: float64, trapezoid rule on the grid `percentiles` (the share of pixels
    dropped), over the rows where both curves are finite (a row that drops every pixel is NaN); NaN with fewer than two.

        AUSE = integral of (curve - oracle)      area of the sparsification error: 0 for an uncertainty that ranks the
                                                 pixels as their errors do
        AURG = integral of (curve[0] - curve)    gain over random removal, whose expected curve is the constant whole-set
                                                 value, i.e. row 0 (nothing dropped)

    so that AUSE + AURG = integral of (curve[0] - oracle), the most any ordering can gain.  `normalize=False` (the default)
    integrates the curves in the unit of the metric, as Poggi et al. 2020 ("On the uncertainty of self-supervised monocular
    depth estimation") report AUSE and AURG; `normalize=True` divides both curves by row 0 first, as Ilg et al. 2018
    ("Uncertainty estimates and multi-hypotheses networks for optical flow") do, whose curves start at 1."""
    x = np.asarray(percentiles, dtype=np.float64)
    c, o = np.asarray(curve, dtype=np.float64), np.asarray(oracle, dtype=np.float64)
    if not (x.shape == c.shape == o.shape and x.ndim == 1):
        raise ValueError("percentiles, curve and oracle must be one-dimensional and of one length")
    ok = np.isfinite(c) & np.isfinite(o)
    if ok.sum() < 2:
        return float("nan"), float("nan")
    x, c, o = x[ok], c[ok], o[ok]
    if normalize:
        c, o = c / c[0], o / o[0]
    w = np.diff(x)
    area = lambda y: float(np.sum(0.5 * (y[1:] + y[:-1]) * w))
    return area(c - o), area(c[0] - c)


def write_sparsification_csv(tables: dict, directory: str) -> Tuple[str, str]:
    """`sparsification.csv` (percentile, then mae_<source> and rmse_<source> per source) and `ause.csv` (one row per
    source) of tables computed with extra sources."""
    os.makedirs(directory, exist_ok=True)
    sp, names = tables["sparsification"], list(tables["sparsification"])
    paths = (os.path.join(directory, "sparsification.csv"), os.path.join(directory, "ause.csv"))
    with open(paths[0], "w") as f:
        f.write(",".join(["percentile"] + [f"{m}_{s}" for s in names for m in ("mae", "rmse")]) + "\n")
        for i, q in enumerate(tables["precision_recall"]["percentile"]):
            f.write(",".join(repr(float(v)) for v in [q] + [sp[s][m][i] for s in names for m in ("mae", "rmse")]) + "\n")
    with open(paths[1], "w") as f:
        f.write("source,ause_mae,ause_rmse,aurg_mae,aurg_rmse\n")
        for s in names:
            row = [tables[a][s][m] for a in ("ause", "aurg") for m in ("mae", "rmse")]
            f.write(s + "," + ",".join(repr(float(v)) for v in row) + "\n")
    return paths


class UncertaintyEvaluator:
    """Streaming reducer of `(mean, aleatoric_var, epistemic_var, label)` batches into the reference's two tables.

    `update` is asynchronous on the current stream; `compute` is the one host synchronisation and may be called
    repeatedly (running tables).  One evaluator is single-stream: `update`, `compute` and `reset` share one workspace
    and one record store, ordered only by the stream they are issued on — call them all under the same current stream.  A single device: to merge evaluators of several GPUs the 65 + 5 accumulators would be
    all-reduced and the three histogram passes all-gathered — not built."""

    def __init__(self, expected_p: Optional[Sequence[float]] = None, percentiles: Optional[Sequence[float]] = None,
                 distribution: str = "norm", clip: Optional[Tuple[float, float]] = (0.0, 1.0), channel: int = 0,
                 device=None, sources: Sequence[str] = ("combined",)):
        self.sources = check_sources(sources)
        # the orderings compute() runs: combined first (the reference's table), the oracle last, and only with extra sources
        extra = self.sources != ("combined",)
        self._orderings = ("combined",) + tuple(s for s in self.sources if s not in ("combined", "oracle")) + (("oracle",) if extra else ())
        self._reported = (self.sources + (() if "oracle" in self.sources else ("oracle",))) if extra else ()
        self._two_stores = any(SOURCES[s][0] == 1 for s in self._orderings)
        self.expected_p = np.arange(41) / 40.0 if expected_p is None else np.asarray(expected_p, dtype=np.float64)
        self.percentiles = np.arange(100) / 100.0 if percentiles is None else np.asarray(percentiles, dtype=np.float64)
        if not 1 <= self.expected_p.size <= MAX_THRESHOLDS or not 1 <= self.percentiles.size <= MAX_PERCENTILES:
            raise ValueError(f"1..{MAX_THRESHOLDS} expected confidences and 1..{MAX_PERCENTILES} percentiles")
        if np.any(np.diff(self.expected_p) < 0) or self.expected_p.min() < 0 or self.expected_p.max() > 1:
            raise ValueError("expected_p must be ascending within [0, 1]")
        self.distribution = distribution
        self.z = standard_quantiles(self.expected_p, distribution)
        self.clip = None if clip is None else (float(clip[0]), float(clip[1]))
        self.channel = int(channel)
        if not torch.cuda.is_available():
            raise L.MimoHipError("UncertaintyEvaluator runs on an AMD GPU (mimo_eval_*); no GPU is visible")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._lib = L.load()
        with torch.cuda.device(self.device):
            self._z_dev = torch.from_numpy(self.z.astype(np.float32)).to(self.device)
            self._pct_dev = torch.from_numpy(np.ascontiguousarray(self.percentiles)).to(self.device)
            self._ws = torch.zeros(int(self._lib.mimo_eval_workspace_bytes()) // 8 + 1, dtype=torch.int64, device=self.device)
            # [3 P + K + 6] of the combined ordering, then one [3 P] slice (mae | rmse | key) per further ordering
            self._out = torch.empty(3 * self.percentiles.size * len(self._orderings) + self.expected_p.size + 6,
                                    dtype=torch.float64, device=self.device)
        self._records = None  # int64 [capacity]: one record per pixel fed
        self._source_records = None  # the second record per pixel (aleatoric_std, epistemic_std), only when asked for
        self._used = 0

    # ------------------------------------------------------------------ feeding
    def reset(self) -> None:
        self._ws.zero_()
        self._used = 0

    def _reserve(self, extra: int) -> None:
        need = self._used + extra
        cap = 0 if self._records is None else self._records.numel()
        if need <= cap:
            return
        for store in ("_records", "_source_records")[: 2 if self._two_stores else 1]:
            grown = torch.empty(max(need, 2 * cap, 1 << 20), dtype=torch.int64, device=self.device)
            if self._used:
                grown[: self._used].copy_(getattr(self, store)[: self._used])  # device to device, on the current stream
            setattr(self, store, grown)

    def update(self, mean, aleatoric_var, epistemic_var, label, mask=None) -> None:
        """Device tensors [B,C,H,W] (mask [B,1,H,W] or [B,C,H,W]).  Enqueues one pass; returns without synchronising."""
        if mean.dim() != 4:
            raise ValueError("update expects [B,C,H,W] tensors")
        b, c, h, w = mean.shape
        if not 0 <= self.channel < c:
            raise ValueError(f"channel {self.channel} of {c}")
        ts = []
        for name, t in (("mean", mean), ("aleatoric_var", aleatoric_var), ("epistemic_var", epistemic_var), ("label", label)):
            if tuple(t.shape) != (b, c, h, w):
                raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {(b, c, h, w)}")
            if not t.is_cuda:
                raise L.MimoHipError(f"UncertaintyEvaluator.update: {name} is not on the GPU (there is no CPU path)")
            ts.append(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        mc = 1
        if mask is not None:
            if mask.dim() != 4 or mask.shape[0] != b or mask.shape[1] not in (1, c) or tuple(mask.shape[2:]) != (h, w):
                raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {(b, 1, h, w)} or {(b, c, h, w)}")
            mc = mask.shape[1]
            mask = mask.detach().to(device=self.device, dtype=torch.float32).contiguous()
        hw = h * w
        with torch.cuda.device(self.device):
            self._reserve(b * hw)
            lo, hi = self.clip if self.clip is not None else (0.0, 0.0)
            if self._two_stores:
                L.check(self._lib.mimo_eval_accumulate_sources(
                    ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), L.ptr(mask) or None, b, c,
                    self.channel, mc, hw, int(self.clip is not None), lo, hi, self._z_dev.data_ptr(), self.z.size,
                    self._records.data_ptr() + 8 * self._used, self._source_records.data_ptr() + 8 * self._used,
                    self._ws.data_ptr(), L.current_stream()), "mimo_eval_accumulate_sources")
            else:
                L.check(self._lib.mimo_eval_accumulate(
                    ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), L.ptr(mask) or None, b, c,
                    self.channel, mc, hw, int(self.clip is not None), lo, hi, self._z_dev.data_ptr(), self.z.size,
                    self._records.data_ptr() + 8 * self._used, self._ws.data_ptr(), L.current_stream()), "mimo_eval_accumulate")
        self._used += b * hw

    def update_from(self, ensemble, image, label, mask=None) -> None:
        """Run an `EnsembleModule` on `image` and feed its `(mean, aleatoric_var, epistemic_var)` without leaving the
        device (the module's `keep_on_device` is switched on for the call).  A bare `EvidentialUnetModel` is fed through its
        `predict_uncertainties` (the reference's scripts/test/test_nyuv2_depth_evidential.py drives the model itself)."""
        from .models.evidential_unet import EvidentialUnetModel
        if isinstance(ensemble, EvidentialUnetModel):
            mean, av, ev = ensemble.predict_uncertainties(image)
            self.update(mean, av, ev, label.to(mean.device), None if mask is None else mask.to(mean.device))
            return
        keep, raw = ensemble.keep_on_device, ensemble.return_raw_predictions
        ensemble.keep_on_device, ensemble.return_raw_predictions = True, False
        try:
            mean, av, ev = ensemble(image)
        finally:
            ensemble.keep_on_device, ensemble.return_raw_predictions = keep, raw
        self.update(mean, av, ev, label.to(mean.device), None if mask is None else mask.to(mean.device))

    # ------------------------------------------------------------------ tables
    def compute(self) -> dict:
        p, k = self.percentiles.size, self.expected_p.size
        if self._used == 0:
            o = np.full(self._out.numel(), np.nan)
            o[3 * p + k: 3 * p + k + 3] = 0.0
        else:
            with torch.cuda.device(self.device):
                s = L.current_stream()
                L.check(self._lib.mimo_eval_select(self._records.data_ptr(), self._used, self._pct_dev.data_ptr(), p,
                                                   self._ws.data_ptr(), s), "mimo_eval_select")
                L.check(self._lib.mimo_eval_interval_sums(self._records.data_ptr(), self._used, p, k, self._ws.data_ptr(),
                                                          self._out.data_ptr(), s), "mimo_eval_interval_sums")
                stores = (self._records, self._source_records)
                errors = self._records.data_ptr() + 4
                for j, name in enumerate(self._orderings[1:]):  # one after another on the one workspace and stream
                    store, word = SOURCES[name]
                    keys = stores[store].data_ptr() + 4 * word
                    L.check(self._lib.mimo_eval_select_by(keys, 2, self._used, self._pct_dev.data_ptr(), p, self._ws.data_ptr(), s),
                            "mimo_eval_select_by")
                    L.check(self._lib.mimo_eval_interval_sums_by(
                        keys, 2, errors, 2, self._used, p, 0, self._ws.data_ptr(),
                        self._out.data_ptr() + 8 * (3 * p * (j + 1) + k + 6), s), "mimo_eval_interval_sums_by")
                o = self._out.cpu().numpy()  # the one transfer (and the one synchronisation)
        n, n_masked, n_nonfinite = (int(v) for v in o[3 * p + k: 3 * p + k + 3])
        if n_nonfinite:
            warnings.warn(f"UncertaintyEvaluator: {n_nonfinite} pixels with a non-finite value or a negative variance were "
                          "skipped (the reference's tables would be NaN in every row)", RuntimeWarning, stacklevel=2)
        tables = {
            "precision_recall": {"percentile": self.percentiles.copy(), "mae": o[:p].copy(), "rmse": o[p: 2 * p].copy()},
            "calibration": {"expected": self.expected_p.copy(), "observed": o[3 * p: 3 * p + k].copy()},
            "cutoff_keys": o[2 * p: 3 * p].copy(),
            "n": n, "n_masked": n_masked, "n_nonfinite": n_nonfinite,
            "mae": float(o[3 * p + k + 3]), "mse": float(o[3 * p + k + 4]), "rmse": float(o[3 * p + k + 5]),
        }
        if self._reported:
            base = {name: 0 if j == 0 else 3 * p * j + k + 6 for j, name in enumerate(self._orderings)}
            sp = {name: {"mae": o[base[name]: base[name] + p].copy(), "rmse": o[base[name] + p: base[name] + 2 * p].copy(),
                         "cutoff_keys": o[base[name] + 2 * p: base[name] + 3 * p].copy()} for name in self._reported}
            areas = {name: {m: sparsification_areas(self.percentiles, sp[name][m], sp["oracle"][m]) for m in ("mae", "rmse")}
                     for name in self._reported}
            tables["sparsification"] = sp
            tables["ause"] = {name: {m: areas[name][m][0] for m in ("mae", "rmse")} for name in self._reported}
            tables["aurg"] = {name: {m: areas[name][m][1] for m in ("mae", "rmse")} for name in self._reported}
        return tables

    def write_csv(self, directory: str, tables: Optional[dict] = None) -> Tuple[str, ...]:
        """The reference's two files; with extra sources also `sparsification.csv` and `ause.csv`."""
        tables = self.compute() if tables is None else tables
        paths = write_tables_csv(tables, directory)
        return paths + write_sparsification_csv(tables, directory) if "sparsification" in tables else paths


# ---------------------------------------------------------------------------------------------------------------------
# Proper scoring rules of the mixture predictive (score_rules.hip)

MAX_MEMBERS = 64            # score_rules.hip: kMaxS
REGISTER_MEMBERS = 4        # score_rules.hip: kRegS — up to here the pair loop runs from registers, beyond from an LDS tile
SCORE_MAX_WORKGROUPS = 1024  # score_rules.hip: kBlocks — a launch's grid; each workgroup strides over the rest
SCORES_HEADER = ("n", "n_masked", "n_nonfinite", "nll", "crps", "pit_mean", "calibration_error")


def check_expected_p(expected_p) -> np.ndarray:
    """The thresholds of a calibration table as float64: 1..64 values, ascending, within [0, 1] (the rule of
    `UncertaintyEvaluator`); the default is `arange(41) / 40`."""
    p = np.arange(41) / 40.0 if expected_p is None else np.asarray(expected_p, dtype=np.float64).reshape(-1)
    if not 1 <= p.size <= MAX_THRESHOLDS:
        raise ValueError(f"1..{MAX_THRESHOLDS} expected confidences")
    if np.any(np.diff(p) < 0) or not (p.min() >= 0 and p.max() <= 1):
        raise ValueError("expected_p must be ascending within [0, 1]")
    return p


def check_score_shapes(p1, p2, label, mask, channel: int) -> Tuple[int, int, int, int, int, int]:
    """(B, S, C, H, W, mask_channels) of one `PredictiveScorer.update`, or ValueError: p1 / p2 [B,S,C,H,W], label
    [B,C,H,W], mask None, [B,1,H,W] or [B,C,H,W], 1 <= S <= 64, 0 <= channel < C."""
    if p1.dim() != 5:
        raise ValueError("update expects p1 and p2 of shape [B,S,C,H,W]")
    b, s, c, h, w = p1.shape
    if tuple(p2.shape) != (b, s, c, h, w):
        raise ValueError(f"p2 has shape {tuple(p2.shape)}, expected {(b, s, c, h, w)}")
    if tuple(label.shape) != (b, c, h, w):
        raise ValueError(f"label has shape {tuple(label.shape)}, expected {(b, c, h, w)}")
    if not 1 <= s <= MAX_MEMBERS:
        raise ValueError(f"{s} members: the mixture is scored for 1..{MAX_MEMBERS}")
    if not 0 <= channel < c:
        raise ValueError(f"channel {channel} of {c}")
    mc = 1
    if mask is not None:
        if mask.dim() != 4 or mask.shape[0] != b or mask.shape[1] not in (1, c) or tuple(mask.shape[2:]) != (h, w):
            raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {(b, 1, h, w)} or {(b, c, h, w)}")
        mc = int(mask.shape[1])
    return b, s, c, h, w, mc


def check_evidential_score_shapes(logits, label, mask) -> Tuple[int, int, int]:
    """(B, H, W) of one `PredictiveScorer.update_evidential`, or ValueError: logits [B,4,H,W], label [B,1,H,W], mask None,
    [B,H,W] or [B,1,H,W]."""
    if logits.dim() != 4 or logits.shape[1] != 4:
        raise ValueError(f"update_evidential expects logits of shape [B,4,H,W], got {tuple(logits.shape)}")
    b, _, h, w = logits.shape
    if tuple(label.shape) != (b, 1, h, w):
        raise ValueError(f"label has shape {tuple(label.shape)}, expected {(b, 1, h, w)}")
    if mask is not None and tuple(mask.shape) not in ((b, h, w), (b, 1, h, w)):
        raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {(b, h, w)} or {(b, 1, h, w)}")
    return int(b), int(h), int(w)


def mixture_of(ensemble) -> Tuple[str, float, float, int]:
    """(loss, eps_min, eps_max, S_total) of the mixture an `EnsembleModule` predicts: S_total = passes x the subnetworks of
    every checkpoint.  A bare `EvidentialUnetModel` raises NotImplementedError (its Student-t predictive needs an
    incomplete-beta CDF); S_total > 64 raises ValueError."""
    from .models.evidential_unet import EvidentialUnetModel
    if isinstance(ensemble, EvidentialUnetModel):
        raise NotImplementedError("PredictiveScorer: the evidential model's Student-t predictive is not scored "
                                  "(its CDF is an incomplete beta function)")
    loss_fn = ensemble.loss_fn
    loss = getattr(loss_fn, "name", "")
    if loss not in L.LOSS_KINDS:
        raise NotImplementedError(f"PredictiveScorer: no mixture density for the loss {type(loss_fn).__name__}")
    s_total = max(1, int(ensemble.monte_carlo_steps)) * int(ensemble.num_subnetworks)
    if s_total > MAX_MEMBERS:
        raise ValueError(f"S_total = {s_total} members: the mixture is scored for at most {MAX_MEMBERS}")
    return loss, float(loss_fn.eps_min), float(loss_fn.eps_max), s_total


def coverage_table(expected_p, observed) -> dict:
    """{level: share} of the central intervals a threshold table holds: every index pair (k, K-1-k) with k < K-1-k and
    |p_k + p_{K-1-k} - 1| <= 1e-12; level = p_{K-1-k} - p_k, share = observed_{K-1-k} - observed_k."""
    p, o = np.asarray(expected_p, dtype=np.float64), np.asarray(observed, dtype=np.float64)
    k_all = p.size
    return {float(p[k_all - 1 - k] - p[k]): float(o[k_all - 1 - k] - o[k]) for k in range(k_all // 2)
            if abs(p[k] + p[k_all - 1 - k] - 1.0) <= 1e-12}


def write_scores_csv(scores: dict, directory: str) -> Tuple[str, str]:
    """`scores.csv` (one row: SCORES_HEADER) and `calibration_mixture.csv` (the reference's calibration header)."""
    os.makedirs(directory, exist_ok=True)
    paths = (os.path.join(directory, "scores.csv"), os.path.join(directory, "calibration_mixture.csv"))
    with open(paths[0], "w") as f:
        f.write(",".join(SCORES_HEADER) + "\n")
        f.write(",".join(repr(int(scores[k])) if k in SCORES_HEADER[:3] else repr(float(scores[k])) for k in SCORES_HEADER) + "\n")
    cal = scores["calibration"]
    with open(paths[1], "w") as f:
        f.write(",".join(CALIBRATION_HEADER) + "\n")
        for row in zip(cal["expected"], cal["observed"]):
            f.write(",".join(repr(float(v)) for v in row) + "\n")
    return paths


class PredictiveScorer:
    """Streaming proper scoring rules of what an ensemble predicts at a pixel: the equal-weight mixture of its S member
    densities (`mimo_score_accumulate`), scored at the label by

        nll        -log of the mixture density, natural log, the FULL density (Laplace -|d|/b - log 2b, Gaussian
                   -d^2/(2 sigma^2) - log sigma - log(2 pi)/2 per member).  This is not the training loss, which drops the
                   constants and, for the Gaussian, a factor 1/2.
        crps       the continuous ranked probability score, closed form for mixtures of Laplace / of Gaussian members
        pit        the probability integral transform u = F(y); its histogram over `expected_p` gives the calibration
                   curve (`observed_k` = share of pixels with u < p_k), its error and the coverage of central intervals

    Member scale as the loss trains it: clamp(exp(p2), eps_min, eps_max) is the Laplace b, or the Gaussian variance.
    Means and labels are NOT clipped — the rules score the distribution as predicted (the tables of `UncertaintyEvaluator`
    clip both to [0, 1] as the reference's scripts do).  A pixel is skipped when mask == 0 (`n_masked`) or when its label or
    any member's p1 / p2 is not finite (`n_nonfinite`).

    The evidential baseline goes through `update_evidential` / `update_from_evidential`: the same three rules of the
    Student-t posterior predictive of its Normal-Inverse-Gamma heads, into the same accumulators (one network: S = 1).

    `update` is asynchronous on the current stream; `compute` is the one host copy.  Single stream, single device, as
    `UncertaintyEvaluator`."""

    def __init__(self, expected_p: Optional[Sequence[float]] = None, channel: int = 0, device=None):
        self.expected_p = check_expected_p(expected_p)
        self.channel = int(channel)
        if not torch.cuda.is_available():
            raise L.MimoHipError("PredictiveScorer runs on an AMD GPU (mimo_score_*); no GPU is visible")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._lib = L.load()
        k = self.expected_p.size
        with torch.cuda.device(self.device):
            self._p_dev = torch.from_numpy(self.expected_p.astype(np.float32)).to(self.device)
            self._ws = torch.zeros(int(self._lib.mimo_score_workspace_bytes()) // 8 + 1, dtype=torch.int64, device=self.device)
            self._out = torch.empty(k + 6, dtype=torch.float64, device=self.device)

    def reset(self) -> None:
        self._ws.zero_()

    def _accumulate(self, p1, p2, label, mask, loss, eps_min, eps_max, maps):
        if loss not in L.LOSS_KINDS:
            raise ValueError(f"loss must be one of {tuple(L.LOSS_KINDS)}, not {loss!r}")
        b, s, c, h, w, mc = check_score_shapes(p1, p2, label, mask, self.channel)
        ts = []
        for name, t in (("p1", p1), ("p2", p2), ("label", label)) + ((("mask", mask),) if mask is not None else ()):
            if not t.is_cuda:
                raise L.MimoHipError(f"PredictiveScorer: {name} is not on the GPU (there is no CPU path)")
            ts.append(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        with torch.cuda.device(self.device):
            out = [torch.empty(b, h, w, dtype=torch.float32, device=self.device) for _ in range(3)] if maps else [None] * 3
            L.check(self._lib.mimo_score_accumulate(
                ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr() if mask is not None else None, b, s, c,
                self.channel, mc, h * w, L.LOSS_KINDS[loss], float(eps_min), float(eps_max), self._p_dev.data_ptr(),
                self.expected_p.size, L.ptr(out[0]) or None, L.ptr(out[1]) or None, L.ptr(out[2]) or None,
                self._ws.data_ptr(), L.current_stream()), "mimo_score_accumulate")
        return tuple(out)

    def update(self, p1, p2, label, mask=None, loss: str = "laplace_nll", eps_min: float = 1e-5, eps_max: float = 1e3) -> None:
        """p1 / p2 [B,S,C,H,W] (the raw member outputs: mean and log-scale), label [B,C,H,W], mask [B,1,H,W] or [B,C,H,W],
        all on the device.  Enqueues one pass; returns without synchronising."""
        self._accumulate(p1, p2, label, mask, loss, eps_min, eps_max, False)

    def score_maps(self, p1, p2, label, mask=None, loss: str = "laplace_nll", eps_min: float = 1e-5, eps_max: float = 1e3):
        """`update`, which also returns the per-pixel (pit, nll, crps) as [B,H,W] device tensors (NaN where skipped)."""
        return self._accumulate(p1, p2, label, mask, loss, eps_min, eps_max, True)

    def update_from(self, ensemble, image, label, mask=None) -> None:
        """Run an `EnsembleModule` on `image` and score the mixture of its raw member outputs without leaving the device;
        the loss kind and its clamps come from `ensemble.loss_fn`."""
        loss, eps_min, eps_max, _ = mixture_of(ensemble)
        keep, raw = ensemble.keep_on_device, ensemble.return_raw_predictions
        ensemble.keep_on_device, ensemble.return_raw_predictions = True, True
        try:
            p1, p2 = ensemble.forward_on_device(image)
        finally:
            ensemble.keep_on_device, ensemble.return_raw_predictions = keep, raw
        self.update(p1, p2, label.to(p1.device), None if mask is None else mask.to(p1.device), loss, eps_min, eps_max)

    # ------------------------------------------------------------------ the evidential model's Student-t predictive
    def _accumulate_evidential(self, logits, label, mask, maps):
        b, h, w = check_evidential_score_shapes(logits, label, mask)
        ts = []
        for name, t in (("logits", logits), ("label", label)) + ((("mask", mask),) if mask is not None else ()):
            if not t.is_cuda:
                raise L.MimoHipError(f"PredictiveScorer: {name} is not on the GPU (there is no CPU path)")
            ts.append(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        with torch.cuda.device(self.device):
            out = [torch.empty(b, h, w, dtype=torch.float32, device=self.device) for _ in range(3)] if maps else [None] * 3
            L.check(self._lib.mimo_score_accumulate_evidential(
                ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr() if mask is not None else None, b, h * w,
                self._p_dev.data_ptr(), self.expected_p.size, L.ptr(out[0]) or None, L.ptr(out[1]) or None,
                L.ptr(out[2]) or None, self._ws.data_ptr(), L.current_stream()), "mimo_score_accumulate_evidential")
        return tuple(out)

    def update_evidential(self, logits, label, mask=None) -> None:
        """logits [B,4,H,W] (the raw outputs of an `EvidentialUnetModel`: `model._logits(image)`), label [B,1,H,W], mask
        [B,H,W] or [B,1,H,W], all on the device.  Scores the Student-t posterior predictive of the Normal-Inverse-Gamma heads
        (nu = 2 alpha, location mu, scale sqrt(beta (1 + v) / (v alpha)); `mimo_score_accumulate_evidential`) into the same
        accumulators as `update`.  A pixel whose v or beta has underflowed to 0 counts as `n_nonfinite`.  Enqueues one pass;
        returns without synchronising.  (The model has one target: `channel` plays no part.)"""
        self._accumulate_evidential(logits, label, mask, False)

    def score_maps_evidential(self, logits, label, mask=None):
        """`update_evidential`, which also returns the per-pixel (pit, nll, crps) as [B,H,W] device tensors (NaN where
        skipped)."""
        return self._accumulate_evidential(logits, label, mask, True)

    def update_from_evidential(self, model, image, label, mask=None) -> None:
        """Run an `EvidentialUnetModel` (in eval mode) on `image` — the no-grad forward on its inference plan — and score
        its logits with one `update_evidential`, without leaving the device.  Anything else is refused with TypeError before
        a kernel is launched (an `EnsembleModule` goes through `update_from`)."""
        from .models.evidential_unet import EvidentialUnetModel
        if not isinstance(model, EvidentialUnetModel):
            raise TypeError(f"PredictiveScorer.update_from_evidential scores an EvidentialUnetModel, not a {type(model).__name__}")
        model.require_eval("PredictiveScorer.update_from_evidential")
        if image.dim() != 4 or image.shape[1] != model.in_channels:
            raise ValueError("channel dimension must match in_channels")
        b, _, h, w = image.shape
        if tuple(label.shape) != (b, 1, h, w):
            raise ValueError(f"label has shape {tuple(label.shape)}, expected {(b, 1, h, w)}")
        if mask is not None and tuple(mask.shape) not in ((b, h, w), (b, 1, h, w)):
            raise ValueError(f"mask has shape {tuple(mask.shape)}, expected {(b, h, w)} or {(b, 1, h, w)}")
        with torch.no_grad():
            logits = model._logits(image.detach())
        self.update_evidential(logits, label.to(logits.device), None if mask is None else mask.to(logits.device))

    def compute(self) -> dict:
        k = self.expected_p.size
        with torch.cuda.device(self.device):
            L.check(self._lib.mimo_score_finalize(self._ws.data_ptr(), k, self._out.data_ptr(), L.current_stream()),
                    "mimo_score_finalize")
            o = self._out.cpu().numpy()  # the one transfer (and the one synchronisation)
        n, n_masked, n_nonfinite = (int(v) for v in o[k: k + 3])
        if n_nonfinite:
            warnings.warn(f"PredictiveScorer: {n_nonfinite} pixels with a non-finite label or member output were skipped",
                          RuntimeWarning, stacklevel=2)
        observed = o[:k].copy()
        return {"n": n, "n_masked": n_masked, "n_nonfinite": n_nonfinite,
                "nll": float(o[k + 3]), "crps": float(o[k + 4]), "pit_mean": float(o[k + 5]),
                "calibration": {"expected": self.expected_p.copy(), "observed": observed},
                "calibration_error": float(np.mean(np.abs(observed - self.expected_p))),
                "coverage": coverage_table(self.expected_p, observed)}

    def write_csv(self, directory: str, scores: Optional[dict] = None) -> Tuple[str, str]:
        """`scores.csv` and `calibration_mixture.csv`."""
        return write_scores_csv(self.compute() if scores is None else scores, directory)
