#!/usr/bin/env python3
"""Capture the adversarial step functions of the sample-index contract from the upstream reference (build container only, CPU).

Run:  python tests/golden/make_golden_sampler_adversarial.py
Needs the reference checkout (see _ref_harness.py).  Arrays and settings only; no reference source travels.

tests/golden/sampler_adversarial.npz
  The reference's stepfun.sample_intervals (stepfun.py:209-258) on the inputs where a CDF inverter goes wrong: ties and plateaus
  of the CDF, -inf logits on zero-length intervals, duplicate knots, one-hot distributions whose CDF saturates before the last
  knot, quantiles exactly on a knot, M and N one off the 64-lane trip count.  Every case is R = 5 rays of one family at one
  (M, N) -- an odd count: the last workgroup of every kernel is partly filled.
    stage_shapes [10, 2], level_shapes [8, 2]    the (M, N) pairs; 512 is the level kernels' n_in limit
  'stage' families: the logits are given.
    stage_families [F]       random, onehot100, onehot40, plateau_inf, front, tail, spread40, uniform, dupknots, clamped
    stage_domain [F, 2]      (smin, smax) of sample_intervals' domain: (0, 1), and (0.2, 0.7) inside the knots for 'clamped'
    stage_s<i>_t [F, R, M + 1], stage_s<i>_logits [F, R, M]
    stage_s<i>_idx [F, R, N] (int16), _sdist [F, R, N + 1], _mask [F, R, N]
  'level' families: weights, anneal and resample_padding are given, the logits are formed as in models.py:200-203.
    level_families [W]       sharp, zeros (runs of exact zeros), onehot, allzero, const
    level_pairs [P, 2]       (anneal, resample_padding): (1, 0.01), (0.3, 0.01), (1, 1e-5), (1, 0), (0, 0.01)
    level_legal [W, P]       False: the combination is not stored (all-zero weights without padding: every logit is -inf)
    level_s<i>_t [2, R, M + 1]        the knots without / with 40 % duplicates
    level_s<i>_w [2, W, R, M]
    level_s<i>_idx [2, W, P, R, N] (int16), _sdist [2, W, P, R, N + 1], _mask [2, W, P, R, N]
  idx is stepfun.searchsorted's idx_lo of every quantile on the reference's own CDF (integrate_weights of its softmax), sdist its
  sample_intervals, mask the quantiles within delta(M) = (M + M / 64 + 9) 2^-24 (tests/helpers.py::cdf_delta) of one of its CDF
  knots: there two fp32 evaluations of the same CDF may take neighbouring bins.

Every input is legal: knots sorted, t[0] = 0 and t[-1] = 1 as the model's first and last edges, at least one finite logit on an
interval of positive length per ray, no NaN.  OUT OF SCOPE: a row of logits that is all -inf (all-zero weights with
resample_padding = 0; a step function all of whose intervals have zero length): the reference's softmax returns NaN there and the
samples are NaN.  anneal = 0 is not combined with resample_padding = 0.
'clamped' is built (clamped_inputs) so that both bounds of its domain bind on every ray -- the reflected end fenceposts lie outside
(0.2, 0.7) and are clamped -- while the reference's edges stay ordered; the script asserts both.  One condition on the draws, read off
the REFERENCE's CDF alone: a draw of duplicate knots over whose positive intervals the uniform distribution has more than 5 % of its
quantiles within delta(M) of a knot is drawn again (level families, N >= 32).

Prints, per family: the share of masked quantiles, the count of bin indices on which the CPU oracle (oracle/refnerf_oracle.c)
differs from the reference inside and outside the mask, and the worst |oracle sdist - reference sdist|.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import _ref_harness  # noqa: E402

_ref_harness.install()
import torch  # noqa: E402

from internal import stepfun  # noqa: E402

from helpers import cdf_delta  # noqa: E402
from oracle import oracle as O  # noqa: E402

R = 5
LEVEL_SHAPES = [(2, 3), (3, 2), (63, 65), (64, 64), (65, 63), (128, 128), (129, 200), (512, 32)]
STAGE_SHAPES = LEVEL_SHAPES + [(257, 129), (1000, 257)]
# (the first seven share one draw of knots per shape: stored next to each other, they compress to one)
STAGE_FAMILIES = ["random", "onehot100", "onehot40", "plateau_inf", "front", "tail", "spread40", "uniform", "dupknots", "clamped"]
LEVEL_FAMILIES = ["sharp", "zeros", "onehot", "allzero", "const"]
LEVEL_PAIRS = [(1.0, 0.01), (0.3, 0.01), (1.0, 1e-5), (1.0, 0.0), (0.0, 0.01)]
NINF = -np.inf


def knots(g, M, dup=0.0):
    """sorted knots from 0 to 1; dup: that share of the intervals has zero length (the last one never)"""
    t = np.sort(g.random((R, M + 1)), -1).astype(np.float32)
    t[:, 0] = 0.0
    if dup:
        for r in range(R):
            for i in np.flatnonzero(g.random(M) < dup):
                t[r, i + 1] = t[r, i]
    t[:, -1] = 1.0
    return t


def runs(g, M, share):
    """a boolean [R, M] that is True on runs of random length covering about `share` of the bins"""
    m = np.zeros((R, M), bool)
    for r in range(R):
        while m[r].mean() < share and not m[r].all():
            i = int(g.integers(0, M))
            m[r, i:i + int(g.integers(1, max(2, M // 8 + 1)))] = True
    return m


def positive_bin(g, t, r):
    """a random interval of positive length of ray r"""
    return int(g.choice(np.flatnonzero(t[r, 1:] > t[r, :-1])))


def clamped_inputs(g, M, N, smin=0.2, smax=0.7):
    """The domain (smin, smax) lies inside the knots and BOTH of its bounds bind on every ray, while the reference's edges stay
    ordered.  Where a bin holds the first two centres they are equally spaced, d = width / (N mass) apart, and the reflected first
    fencepost 1.5 c0 - 0.5 c1 is the bin's lower knot; likewise at the far end.  So: no mass before t[1] and after t[M-1], the first
    and the last bin with mass wide ([t[1], >= 0.3], [<= 0.6, t[M-1]]) and holding two centres (mass 2 / N, as every bin with mass),
    t[1] = smin - a with 0 < a < d (the first fencepost is clamped up to smin, the next edge t[1] + d stays above it), t[M-1] =
    smax + b likewise.  M = 2 has no interior bin: knots (0, x, 1), masses (p, 1 - p) with x, p near 0.6 put two of the three centres
    into [0, x] (first fencepost 0, clamped; next edge x / (3 p) > smin) and the last reflects beyond smax."""
    t = np.zeros((R, M + 1), np.float64)
    t[:, -1] = 1.0
    if M == 2:
        t[:, 1] = 0.58 + 0.04 * g.random(R)
        p = 0.58 + 0.04 * g.random(R)
        return t.astype(np.float32), np.log(np.stack([p, 1.0 - p], -1))
    t[:, 2:M - 1] = np.sort(0.3 + 0.3 * g.random((R, M - 3)), -1)
    # K = N / 2 of the interior bins carry mass, the same each (the others are plateaus of the CDF): two centres per bin, and 1 / K and
    # its running sum are the same numbers in the reference and in the oracle -- this family's index equality holds for every draw
    K = max(1, min(M - 2, N // 2))
    lg = np.full((R, M), NINF)
    for r in range(R):
        lg[r, np.r_[1, M - 2, 2 + g.permutation(max(M - 4, 0))[:max(K - 2, 0)]].astype(int)] = 0.0
    mass = np.full((R, 2), 1.0 / np.isfinite(lg).sum(-1)[:, None])
    assert (mass > 1.6 / N).all()                                # u_1 = 1.5 / N lies inside the first bin with mass
    lo_end = t[:, 2] if M > 3 else np.full(R, smax)            # the other knot of the first / last bin with mass, before t[1], t[M-1] move out
    hi_end = t[:, M - 2] if M > 3 else np.full(R, smin)
    t[:, 1] = smin - (0.3 + 0.4 * g.random(R)) * (lo_end - smin) / (N * mass[:, 0])
    t[:, M - 1] = smax + (0.3 + 0.4 * g.random(R)) * (smax - hi_end) / (N * mass[:, -1])
    return t.astype(np.float32), lg


def stage_inputs(fam, g, M, N, shared_t):
    """-> t [R, M + 1], logits [R, M]"""
    t = knots(g, M, dup=0.4) if fam == "dupknots" else shared_t.copy()
    if fam in ("random", "dupknots"):
        lg = 3.0 * g.standard_normal((R, M))
    elif fam == "clamped":
        t, lg = clamped_inputs(g, M, N)
    elif fam == "uniform":                       # exact binary fractions where M is a power of two: quantiles ON knots
        t = np.tile(np.linspace(0, 1, M + 1, dtype=np.float32), (R, 1))
        lg = np.zeros((R, M))
    elif fam in ("onehot100", "onehot40"):       # exp(-100) underflows fp32: the CDF is 0 ... 0 1 ... 1; exp(-40) does not
        lg = np.full((R, M), -100.0 if fam == "onehot100" else -40.0)
        for r in range(R):
            lg[r, 0 if r == 0 else (M - 1 if r == 1 else int(g.integers(0, M)))] = 0.0
    elif fam == "plateau_inf":                   # 60 % of the bins without mass, in runs
        lg = 3.0 * g.standard_normal((R, M))
        lg[runs(g, M, 0.6)] = NINF
        for r in range(R):
            lg[r, int(g.integers(0, M))] = g.standard_normal()
    elif fam in ("front", "tail"):               # all mass within a few bins of one end
        lg = -1.5 * np.tile(np.arange(M, dtype=np.float64), (R, 1)) + 0.3 * g.standard_normal((R, M))
        lg = lg if fam == "front" else lg[:, ::-1]
    elif fam == "spread40":
        lg = 40.0 * g.standard_normal((R, M))
    else:
        raise KeyError(fam)
    lg = np.where(t[:, 1:] > t[:, :-1], lg, NINF).astype(np.float32)      # zero-length intervals as the model hands them on
    return t, lg


def level_weights(fam, g, t):
    M = t.shape[1] - 1
    if fam in ("sharp", "zeros"):
        w = g.random((R, M)) ** 8
        w = 0.9 * w / w.sum(-1, keepdims=True)
        if fam == "zeros":
            w[runs(g, M, 0.5)] = 0.0
            w[:, -1] = 0.05                      # (the last interval always has positive length)
    elif fam == "onehot":
        w = np.zeros((R, M))
        for r in range(R):
            w[r, positive_bin(g, t, r)] = 1.0
    elif fam == "allzero":
        w = np.zeros((R, M))
    elif fam == "const":
        w = np.full((R, M), 1.0 / M)
    else:
        raise KeyError(fam)
    return w.astype(np.float32)


def reference(t, logits, N, smin, smax):
    """the reference's CDF bin index of every quantile, its sdist, and the mask of the quantiles near one of its CDF knots"""
    M = logits.shape[1]
    tt, lg = torch.tensor(t), torch.tensor(logits)
    assert bool((tt[:, 1:] >= tt[:, :-1]).all()) and not bool(torch.isnan(lg).any())
    assert bool(((lg > NINF) & (tt[:, 1:] > tt[:, :-1])).any(-1).all()), "a ray without a finite logit on a positive interval"
    sd = stepfun.sample_intervals(tt, lg, N, single_jitter=False, domain=(smin, smax), use_gpu_resampling=False)
    assert not bool(torch.isnan(sd).any())
    eps = torch.finfo(torch.float32).eps
    pad = 1 / (2 * N)
    u = torch.linspace(pad, 1.0 - pad - eps, N)                          # stepfun.py:199-201
    cw = stepfun.integrate_weights(torch.softmax(lg, dim=-1))
    idx, _ = stepfun.searchsorted(cw, u.expand(R, N))
    near = (u.double()[None, :, None] - cw.double()[:, None, :]).abs().min(-1).values <= cdf_delta(M)
    return idx.numpy().astype(np.int16), sd.numpy(), near.numpy()


class Table:
    def __init__(self):
        self.rows = {}

    def add(self, fam, t, logits, N, smin, smax, idx, sd, mask):
        sd_o, idx_o = O.sample_intervals(t, logits, N, smin=smin, smax=smax)
        diff = idx_o != idx
        clean = ~mask.any(-1)
        row = self.rows.setdefault(fam, dict(n=0, masked=0, inside=0, outside=0, sd=0.0, sd_clean=0.0))
        row["n"] += mask.size
        row["masked"] += int(mask.sum())
        row["inside"] += int((diff & mask).sum())
        row["outside"] += int((diff & ~mask).sum())
        row["sd"] = max(row["sd"], float(np.abs(sd_o - sd).max()))
        if clean.any():
            row["sd_clean"] = max(row["sd_clean"], float(np.abs(sd_o - sd)[clean].max()))

    def show(self, title):
        print(title)
        print(f"  {'family':<12} {'quantiles':>9} {'masked':>8} {'idx != ref in mask':>19} {'outside':>8} {'max |sdist - ref|':>18} {'on unmasked rays':>17}")
        for fam, r in self.rows.items():
            print(f"  {fam:<12} {r['n']:>9} {100 * r['masked'] / r['n']:>7.2f}% {r['inside']:>19} {r['outside']:>8} {r['sd']:>18.2e} {r['sd_clean']:>17.2e}")


def main():
    out = dict(stage_shapes=np.array(STAGE_SHAPES, np.int32), level_shapes=np.array(LEVEL_SHAPES, np.int32),
               stage_families=np.array(STAGE_FAMILIES), level_families=np.array(LEVEL_FAMILIES),
               level_pairs=np.array(LEVEL_PAIRS, np.float32),
               stage_domain=np.array([(0.2, 0.7) if f == "clamped" else (0.0, 1.0) for f in STAGE_FAMILIES], np.float32))
    legal = np.ones((len(LEVEL_FAMILIES), len(LEVEL_PAIRS)), bool)
    legal[LEVEL_FAMILIES.index("allzero"), LEVEL_PAIRS.index((1.0, 0.0))] = False
    out["level_legal"] = legal
    stage_table, level_table = Table(), Table()
    for s, (M, N) in enumerate(STAGE_SHAPES):
        acc = {k: [] for k in ("t", "logits", "idx", "sdist", "mask")}
        shared_t = knots(np.random.default_rng([11, s]), M)
        for f, fam in enumerate(STAGE_FAMILIES):
            smin, smax = (float(v) for v in out["stage_domain"][f])
            # One draw per family and shape, the seed below: the reference's own edges must come out ordered and inside the domain.
            # The stage families' indices are asserted equal to the reference's at EVERY quantile; that holds for these seeds and is
            # not a property of every draw: the oracle's softmax (shared exp, sequential fp32 sum, division) and torch's (vectorised)
            # differ by ulps, so with other seeds expect a few quantiles within some ulp of a CDF knot, at M = 1000 above all, in
            # neighbouring bins (the 'idx != ref in mask' column below) -- neither an oracle bug nor a kernel bug.
            t, lg = stage_inputs(fam, np.random.default_rng([11, s, f, 0]), M, N, shared_t)
            idx, sd, mask = reference(t, lg, N, smin, smax)
            assert (np.diff(sd, axis=-1) >= 0).all() and sd.min() >= smin and sd.max() <= smax, f"{fam} {M}x{N}: the reference's edges"
            if fam == "clamped":
                assert (sd[:, 0] == np.float32(smin)).all() and (sd[:, -1] == np.float32(smax)).all(), f"clamped {M}x{N}: a bound does not bind"
            stage_table.add(fam, t, lg, N, smin, smax, idx, sd, mask)
            for k, v in zip(acc, (t, lg, idx, sd, mask)):
                acc[k].append(v)
        for k, v in acc.items():
            out[f"stage_s{s}_{k}"] = np.stack(v)
    for s, (M, N) in enumerate(LEVEL_SHAPES):
        ts, ws = [], []
        idx = np.zeros((2, len(LEVEL_FAMILIES), len(LEVEL_PAIRS), R, N), np.int16)
        sd = np.zeros((2, len(LEVEL_FAMILIES), len(LEVEL_PAIRS), R, N + 1), np.float32)
        mask = np.zeros(idx.shape, bool)
        for d in range(2):
            for attempt in range(200):
                g = np.random.default_rng([13, s, d, attempt])
                t = knots(g, M, dup=0.4 * d)
                # a draw of duplicates over whose positive intervals the UNIFORM distribution (constant or all-zero weights, anneal = 0)
                # has more than 5 % of its quantiles within delta(M) of a knot is drawn again (N >= 32; without duplicates M and N decide)
                uniform = np.where(t[:, 1:] > t[:, :-1], 0.0, NINF).astype(np.float32)
                if d == 0 or N < 32 or reference(t, uniform, N, 0.0, 1.0)[2].mean() <= 0.05:
                    break
            else:
                raise RuntimeError(f"level {M}x{N}: no legal draw of duplicate knots")
            ts.append(t)
            ws.append(np.stack([level_weights(fam, g, t) for fam in LEVEL_FAMILIES]))
            for f, fam in enumerate(LEVEL_FAMILIES):
                for p, (anneal, padding) in enumerate(out["level_pairs"]):
                    if not legal[f, p]:
                        continue
                    tt, ww = torch.tensor(t), torch.tensor(ws[d][f])
                    lg = torch.where(tt[..., 1:] > tt[..., :-1], float(anneal) * torch.log(ww + float(padding)), -float("inf")).numpy()   # models.py:200-203
                    idx[d, f, p], sd[d, f, p], mask[d, f, p] = reference(t, lg, N, 0.0, 1.0)
                    # the oracle forms its own logits (the shared rn_det_logf): its indices may differ inside the mask
                    level_table.add(fam, t, O.resample_logits(t, ws[d][f], float(anneal), float(padding)), N, 0.0, 1.0,
                                    idx[d, f, p], sd[d, f, p], mask[d, f, p])
        out[f"level_s{s}_t"], out[f"level_s{s}_w"] = np.stack(ts), np.stack(ws)
        out[f"level_s{s}_idx"], out[f"level_s{s}_sdist"], out[f"level_s{s}_mask"] = idx, sd, mask
    stage_table.show("stage families (logits given): the oracle against the reference")
    level_table.show("level families (weights, anneal, padding given): the oracle, with its own logits, against the reference")
    path = os.path.join(HERE, "sampler_adversarial.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
