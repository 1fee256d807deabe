"""GPU: the sample-index contract (README) on adversarial step functions.

tests/golden/sampler_adversarial.npz holds what a CDF inverter gets wrong -- ties and plateaus of the CDF (runs of bins without
mass), -inf logits on zero-length intervals, duplicate knots, one-hot distributions whose CDF saturates at 1 before the last
knot, quantiles on knots, a domain inside the knots, M and N one off the 64-lane trips of rn::build_cdf_wave -- with the
reference's own bin indices and sdist.  Here every kernel that resamples is fed every case it can hold:
  * the sampler stage: bin_idx and sdist bit-equal to the CPU oracle's, indices equal to the reference's;
  * the level kernels whose CDF is the sequential one (resample_phase<..., true>: f32 eval and training, f16x2 eval, the split-f16
    and the bf16-chain training forwards): bit-equal to the oracle's on (sdist_in, weights_in, anneal, resample_padding);
  * what those rays then render in the two parity modes, against the float64 build of the oracle;
  * the throughput modes (bf16, f16), whose CDF is summed wave-parallel: equal up to the summation order, with the bound derived.
Five rays per launch, the fixture's shapes only."""
import functools

import numpy as np
import pytest
import torch

from helpers import adversarial_cases, cdf_delta, load_golden
from oracle import oracle as O
from refnerf_pl_amd import _hip, synthetic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = 5
PARAM_KW = dict(seed=3, bias_scale=0.05, sharpen=8.0)           # the random-init weights of tests/test_guard_bands.py
SCRATCH_REFUSAL = "too large for the resampler scratch of this precision mode"
MUST_RUN_UP_TO = (129, 200)                                      # ... and every smaller pair runs in every mode


def _shapes(kind):
    return [(int(M), int(N)) for M, N in load_golden("sampler_adversarial")[kind + "_shapes"]]


def _ids(shapes):
    return ["%dx%d" % s for s in shapes]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _stop_on_hip_error(fn, what):
    """a HIP runtime error is a device fault: nothing more is started on this device"""
    try:
        return fn()
    except (_hip.HipLibraryError, RuntimeError) as e:
        if isinstance(e, _hip.HipLibraryError) or "hip error" in str(e).lower():
            pytest.exit(f"{what}: the HIP runtime reported an error; nothing more is started on this device: {e}", returncode=3)
        raise


@functools.lru_cache(maxsize=None)
def _oracle_stage(kind, shape):
    """[(case, logits, the oracle's sdist, bin_idx)] of one shape: computed once, shared, left unchanged"""
    out = []
    for c in adversarial_cases(kind, shape):
        lg = c["logits"] if kind == "stage" else O.resample_logits(c["t"], c["w"], c["anneal"], c["padding"])
        out.append((c, lg) + O.sample_intervals(c["t"], lg, c["N"], smin=c["smin"], smax=c["smax"]))
    return out


# ------------------------------------------------------------------------------------------------- the sampler stage
@pytest.mark.parametrize("kind,shape", [(k, s) for k in ("stage", "level") for s in _shapes(k)],
                         ids=[f"{k}-{i}" for k in ("stage", "level") for i in _ids(_shapes(k))])
def test_stage_bit_equal_to_the_oracle_and_indices_equal_to_the_reference(kind, shape):
    """refnerf_sample_intervals on every case (the level families with the logits of O.resample_logits): bin_idx and sdist are
    bit-equal to the oracle's; on the stage families the indices are the reference's, on the level families (logits an ulp from
    torch's) outside the mask of the quantiles within cdf_delta(M) of a reference CDF knot."""
    _hip.require_device()
    for c, lg, sd_o, idx_o in _oracle_stage(kind, shape):
        sd, idx = _stop_on_hip_error(lambda: _hip.sample_intervals(T(c["t"]), T(lg), c["N"], c["smin"], c["smax"]), c["id"])
        sd, idx = sd.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(idx, idx_o), f"{c['id']}: {int((idx != idx_o).sum())} bin indices differ from the oracle's"
        assert np.array_equal(sd, sd_o), f"{c['id']}: sdist is not bit-equal to the oracle's"
        keep = np.ones_like(c["mask"]) if kind == "stage" else ~c["mask"]
        assert np.array_equal(idx[keep], c["idx"][keep]), f"{c['id']}: {int((idx != c['idx'])[keep].sum())} bin indices differ from the reference's"
        assert np.all(np.diff(sd, axis=-1) >= 0) and sd.min() >= c["smin"] and sd.max() <= c["smax"], c["id"]


# ------------------------------------------------------------------------------------------------- the level kernels
# mode -> (precision, training, wgrad_mode): the forwards whose CDF is the oracle's sequential one
EXACT_MODES = {"f32-eval": ("PREC_F32", False, None), "f32-train": ("PREC_F32", True, None),
               "f16x2-eval": ("PREC_F16X2", False, None),
               "f16x2-train": ("PREC_F16X2", True, "WGRAD_BF16X3"), "f16x2-train-wgradf16": ("PREC_F16X2", True, "WGRAD_F16"),
               "bf16-train": ("PREC_BF16", True, None)}
THROUGHPUT_MODES = {"bf16-eval": ("PREC_BF16", False, None), "f16-eval": ("PREC_F16", False, None)}
GATE_K = {"f32-eval": 2.0, "f16x2-eval": 4.0}                    # the float64 gate's factor per mode


@functools.lru_cache(maxsize=None)
def _rays():
    return synthetic.blender_rays(R, seed=R, center_frac=0.5)


@functools.lru_cache(maxsize=None)
def _dev_rays():
    return {k: (T(_rays()[k]).reshape(-1) if k in ("radii", "near", "far") else T(_rays()[k]))
            for k in ("origins", "directions", "viewdirs", "radii", "near", "far")}


@functools.lru_cache(maxsize=None)
def _image(kind):
    return _hip.pack_weights(T(synthetic.make_params(**PARAM_KW)), precision=kind)


@functools.lru_cache(maxsize=None)
def _hip_levels(mode, shape):
    """[(case, outputs as numpy | the library's ValueError)] of one mode at one shape: launched once, shared by the tests below"""
    _hip.require_device()
    prec, training, wgrad = {**EXACT_MODES, **THROUGHPUT_MODES}[mode]
    prec = getattr(_hip, prec)
    out = []
    for c in adversarial_cases("level", shape):
        kw = dict(n_samples=c["N"], n_in=c["M"], precision=prec, training=int(training), anneal=c["anneal"], resample_padding=c["padding"])
        if wgrad is not None:
            kw["wgrad_mode"] = getattr(_hip, wgrad)
        cfg = _hip.default_cfg(**kw)

        def run():
            try:
                res = _hip.level_forward(_image(_hip.level_image(prec, training, 0)), cfg, _dev_rays(), T(c["t"]), T(c["w"]),
                                         save_activations=training)
            except ValueError as e:
                return e
            return {k: v.cpu().numpy() for k, v in res.items() if torch.is_tensor(v) and k != "activations"}
        out.append((c, _stop_on_hip_error(run, f"{mode} {c['id']}")))
    return out


def _ran(mode, c, res):
    """True where the level ran; a shape the mode's resampler scratch cannot hold is refused with the library's ValueError and
    nothing else, and only beyond (129, 200)"""
    if not isinstance(res, ValueError):
        return True
    assert SCRATCH_REFUSAL in str(res), f"{mode} {c['id']}: refused with {res!r}"
    assert not (c["M"] <= MUST_RUN_UP_TO[0] and c["N"] <= MUST_RUN_UP_TO[1]), f"{mode} {c['id']}: must run, was refused: {res}"
    return False


@pytest.mark.parametrize("mode", list(EXACT_MODES))
@pytest.mark.parametrize("shape", _shapes("level"), ids=_ids(_shapes("level")))
def test_exact_level_kernels_bit_equal_to_the_oracle(shape, mode):
    """every forward that instantiates resample_phase<..., true>, fed every level case as (sdist_in, weights_in) with cfg.anneal,
    cfg.resample_padding and n_in: bin_idx and sdist are bit-equal to O.sample_intervals(t, O.resample_logits(t, w, anneal,
    padding), N)"""
    ran = 0
    for (c, res), (_, _, sd_o, idx_o) in zip(_hip_levels(mode, shape), _oracle_stage("level", shape)):
        if not _ran(mode, c, res):
            continue
        ran += 1
        assert np.array_equal(res["bin_idx"], idx_o), f"{mode} {c['id']}: {int((res['bin_idx'] != idx_o).sum())} bin indices differ from the oracle's"
        assert np.array_equal(res["sdist"], sd_o), f"{mode} {c['id']}: sdist is not bit-equal to the oracle's"
    print(f"MEASURED {mode} {shape}: {ran} of {len(_hip_levels(mode, shape))} cases ran, the others were refused for the resampler scratch")


@functools.lru_cache(maxsize=None)
def _oracle_levels(shape):
    """[(fp32 oracle, float64 oracle)] level_forward of every level case of one shape on the rays and weights the kernels get"""
    from oracle import oracle_f64 as O64
    P, rays = synthetic.make_params(**PARAM_KW), _rays()
    out = []
    for c in adversarial_cases("level", shape):
        kw = dict(n_samples=c["N"], n_in=c["M"], anneal=c["anneal"], resample_padding=c["padding"])
        out.append(tuple(o.level_forward(P, o.default_cfg(**kw), rays, c["t"], c["w"], history=False) for o in (O, O64)))
    return out


@pytest.mark.parametrize("mode", list(GATE_K))
@pytest.mark.parametrize("shape", _shapes("level"), ids=_ids(_shapes("level")))
def test_what_the_rays_render_against_float64(shape, mode):
    """the two parity modes: per-sample weights, r_rgb and r_acc of the same launches against the oracle's level_forward on the
    same inputs, through the project's gate against the float64 build: |hip - f64| <= max(1e-5, K |fp32 oracle - f64|), K = 2 for
    the f32 mode, 4 for f16x2.  The bins are the oracle's (the test above), so no ray is left out; samples
    crowded into one narrow bin have tiny intervals and near-zero variances, which is the point.  Every value is finite."""
    k = GATE_K[mode]
    worst = {}
    for (c, res), (o32, o64) in zip(_hip_levels(mode, shape), _oracle_levels(shape)):
        if not _ran(mode, c, res):
            continue
        assert np.array_equal(res["bin_idx"], o32["bin_idx"]), f"{mode} {c['id']}: the bins are not the oracle's"
        for key in ("weights", "r_rgb", "r_acc"):
            hip = res[key].astype(np.float64)
            assert np.all(np.isfinite(hip)), f"{mode} {c['id']} {key}: not finite"
            e, er = np.abs(hip - o64[key].reshape(hip.shape)), np.abs(o32[key].reshape(hip.shape).astype(np.float64) - o64[key].reshape(hip.shape))
            bound = np.maximum(1e-5, k * er)
            w = worst.setdefault(key, [0.0, 0.0, 0.0, ""])
            if float((e / bound).max()) > w[2]:
                w[2], w[3] = float((e / bound).max()), c["id"]
            w[0], w[1] = max(w[0], float(e.max())), max(w[1], float(er.max()))
    for key, (e, er, ratio, cid) in worst.items():
        print(f"MEASURED {mode} {shape} {key}: max |hip - f64| {e:.2e}, max |fp32 oracle - f64| {er:.2e}, largest share of the gate {ratio:.2f} ({cid})")
    for key, (e, er, ratio, cid) in worst.items():
        assert ratio <= 1.0, f"{mode} {key}: {ratio:.2f} of the gate on {cid}"


# ------------------------------------------------------------------------------------------------- the throughput modes
THROUGHPUT_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def _throughput_families():
    """the level families of which at most 1 % of the quantiles are masked in the fixture: not the uniform ones (constant or
    all-zero weights), whose quantiles sit on knots by construction"""
    cases = adversarial_cases("level")
    fams = []
    for fam in dict.fromkeys(c["family"] for c in cases):
        m = [c["mask"] for c in cases if c["family"] == fam]
        if sum(int(x.sum()) for x in m) <= THROUGHPUT_SHARE * sum(x.size for x in m):
            fams.append(fam)
    return fams


@pytest.mark.parametrize("mode", list(THROUGHPUT_MODES))
@pytest.mark.parametrize("shape", _shapes("level"), ids=_ids(_shapes("level")))
def test_throughput_modes_equal_up_to_the_summation_order(shape, mode):
    """bf16 and f16 eval levels sum the CDF wave-parallel (build_cdf_wave<false>): the same terms in another order.
    How far the two CDFs can lie apart at a knot, in units of 2^-24 (half an ulp below 1; every term and partial sum is <= 1):
    the sequential fp32 sum of the M softmax terms M (one rounding per addition), the tree over the same terms M / 64 + 6 (M / 64
    additions per lane, six butterfly steps), the division by either sum, the float64 running sum's final rounding to fp32 and the
    division of the other side 3 -- together cdf_delta(M) = (M + M / 64 + 9) 2^-24.  So
      * a quantile within cdf_delta(M) of an ORACLE knot may take the neighbouring bin and is left out; elsewhere bin_idx is the
        oracle's;
      * a centre c = t[lo] + off (t[lo+1] - t[lo]), off = (u - cw[lo]) / (cw[lo+1] - cw[lo]) clipped to [0, 1], moves by at most
        (t[lo+1] - t[lo]) min(1, 2 delta / (cw[lo+1] - cw[lo])) -- both knots of the bin move by up to delta --, plus 4 ulp of the
        knot range for the fp32 evaluation of the expression on either side;
      * sdist, averages of neighbouring centres and the clamped reflected ends, lies within the larger of the bounds of the two
        centres it is made of, where neither is masked; it is ordered and inside [s_near, s_far].
    The level kernels hand out sdist, not the centres, so the centre bound is asserted through the sdist bound only.  For the interior
    edges (c[k-1] + c[k]) / 2 the larger of the two bounds is derived; for the two end fenceposts, 1.5 c0 - 0.5 c1 where not clamped,
    the derived bound is 1.5 b0 + 0.5 b1, up to twice as much: there max(b0, b1) is the statement this test was given, kept as the
    tighter of the two and measured against (largest share of it on an MI355X: 0.29), not derived.
    Only families of which at most 1 % of the quantiles are masked run: no constant or all-zero weights."""
    fams = _throughput_families()
    assert "const" not in fams and "allzero" not in fams and {"sharp", "zeros", "onehot"} <= set(fams), fams
    delta = cdf_delta(shape[0])
    worst_sd, worst_share, left_out, total = 0.0, 0.0, 0, 0
    for (c, res), (_, lg, sd_o, idx_o) in zip(_hip_levels(mode, shape), _oracle_stage("level", shape)):
        if c["family"] not in fams or not _ran(mode, c, res):
            continue
        t, N = c["t"].astype(np.float64), c["N"]
        cw = O.resample_cdf(lg).astype(np.float64)
        u = O.linspace_u(N).astype(np.float64)
        near = np.abs(u[None, :, None] - cw[:, None, :]).min(-1) <= delta               # [R, N]: within delta of an oracle knot
        keep = ~near
        left_out, total = left_out + int(near.sum()), total + near.size
        assert np.array_equal(res["bin_idx"][keep], idx_o[keep]), f"{mode} {c['id']}: {int((res['bin_idx'] != idx_o)[keep].sum())} bin indices differ away from a knot"
        lo = idx_o.astype(np.int64)
        take = lambda a, i: np.take_along_axis(a, i, axis=-1)                            # noqa: E731
        width, mass = take(t, lo + 1) - take(t, lo), take(cw, lo + 1) - take(cw, lo)
        assert np.all(mass > 0)
        ulp = np.spacing((c["t"][:, -1] - c["t"][:, 0]).astype(np.float32)).astype(np.float64)[:, None]
        b = width * np.minimum(1.0, 2.0 * delta / mass) + 4.0 * ulp                      # [R, N]: the bound of every centre
        # sdist[k] is made of the centres k - 1 and k; the two ends of the centres 0, 1 and N - 2, N - 1
        first, second = np.r_[0, np.arange(N - 1), N - 2], np.r_[1, np.arange(1, N), N - 1]
        bound = np.maximum(b[:, first], b[:, second])
        ok = keep[:, first] & keep[:, second]
        sd = res["sdist"].astype(np.float64)
        err = np.abs(sd - sd_o)
        if ok.any():
            worst_sd, worst_share = max(worst_sd, float(err[ok].max())), max(worst_share, float((err[ok] / bound[ok]).max()))
        assert np.all(err[ok] <= bound[ok]), f"{mode} {c['id']}: |sdist - oracle| is {float((err[ok] / bound[ok]).max()):.2f} of its bound"
        assert np.all(np.diff(res["sdist"], axis=-1) >= 0), f"{mode} {c['id']}: sdist decreases"
        assert res["sdist"].min() >= 0.0 and res["sdist"].max() <= 1.0, f"{mode} {c['id']}"
    print(f"MEASURED {mode} {shape}: {left_out} of {total} quantiles within cdf_delta of an oracle knot left out; "
          f"max |sdist - oracle| {worst_sd:.2e}, largest share of its bound {worst_share:.2f}")
