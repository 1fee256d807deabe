"""GPU: the per-sample phases of the split-f16 eval kernel (`level_fwd_split` in csrc/refnerf_level_bf16.h) that do no matrix
work -- P1 (IPE, four lanes per sample), layer 0's B fragments, P4 (head activations, evaluated once and parked in the sample's
record by one lane of the sample) and P6 (colours, the sample's two lanes taking a column each).  Every one of them maps
samples to lanes, half-waves and 16-sample runs by hand, so a mistake writes a value from the wrong lane: wrong by orders of
magnitude, for some placements of a ray only.  Two kinds of check:

  * every per-ray rendering and every per-sample history array against the CPU oracle, on batches that fill passes and
    workgroups in different ways (full workgroups, a half-filled pass, a partly filled last workgroup, passes that end
    inside a ray, two passes per workgroup);
  * the same rays in another order: each ray lands on other waves, and (72 samples per ray) on the other 16-sample run and
    on other lanes.  The MLP of a sample depends on nothing but the sample and the per-ray phases run one ray per wave, so
    after un-permuting every array is equal bit for bit.

Tolerance against the oracle: the parity bar of the f16x2 mode (tests/test_hip_f16x2.py: 1e-4 on rendered RGB and on the
compositing weights), applied as |hip - oracle| <= 1e-4 * max(1, |oracle|): absolute for what is bounded by one (colours,
tint, weights, sdist, acc), relative for what is not (density, roughness, grad_pred, distance).  The spatial operands carry
22 significand bits (2.4e-7) through eight 256-wide layers; measured errors of the mode are 1e-6 .. 1e-5.  normals_pred =
-grad_pred / |grad_pred| amplifies grad_pred's error by 2 / |grad_pred| where the predicted gradient is short, so its bar
is 2e-4 * max(1, 1 / |grad_pred|).  Level 0's sdist does not depend on the MLP: bit-equal.  Per-sample arrays are compared on
the rays whose level-1 bin indices equal the oracle's (a quantile within an ulp of a CDF knot may take the neighbouring bin
and move the sample: tests/test_hip_parity.py)."""
import numpy as np
import pytest

from refnerf_pl_amd import synthetic
from test_hip_parity import DEV, O, hip, run_hip_model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F16X2 = 3
TOL = 1e-4
PER_SAMPLE = ("density", "roughness", "rgb", "diffuse", "specular", "normals_pred", "grad_pred", "tint", "weights", "sdist")
_BLOB = synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0)
_RAYS = synthetic.blender_rays(2048, seed=21, center_frac=0.5)
_hip_cache, _oracle_cache = {}, {}


def take(idx):
    return {k: v[idx] for k, v in _RAYS.items()}


def render(hip, idx, n_samples, key=None):
    """both levels of the rays _RAYS[idx] in f16x2 (computed once per module for a given `key`)"""
    if key is None or key not in _hip_cache:
        lv = dict(num_prop_samples=n_samples, num_nerf_samples=n_samples)
        out = run_hip_model(hip, _BLOB, take(idx), {}, lv, precision=F16X2)
        if key is None:
            return out
        _hip_cache[key] = out
    return _hip_cache[key]


def oracle(O, n_rays, n_samples):
    key = (n_rays, n_samples)
    if key not in _oracle_cache:
        _oracle_cache[key] = O.model_forward(_BLOB, take(slice(0, n_rays)), num_prop_samples=n_samples, num_nerf_samples=n_samples)
    return _oracle_cache[key]


def bar(name, ref, ref_level):
    """largest admissible |hip - oracle| per element (module docstring)"""
    if name == "normals_pred":
        gl = np.sqrt((ref_level["grad_pred"].astype(np.float64) ** 2).sum(-1, keepdims=True))
        return 2 * TOL * np.maximum(1.0, 1.0 / np.maximum(gl, 1e-30))
    return TOL * np.maximum(1.0, np.abs(ref))


@pytest.mark.parametrize("batch,n_rays,n_samples", [(9, 9, 128), (5, 5, 192), (6, 6, 64), (2048, 16, 128)],
                         ids=["9x128", "5x192", "6x64", "first16_of_2048x128"])
def test_all_outputs_vs_oracle(hip, O, batch, n_rays, n_samples):
    """9 x 128: full workgroups (two rays = one pass) plus a half-filled pass in a partly filled last workgroup; 5 x 192:
    passes that end inside a ray; 6 x 64; the first 16 rays of 2048 x 128: four rays per workgroup, two passes."""
    out = render(hip, np.arange(batch), n_samples, key=(batch, n_samples))
    ref = oracle(O, n_rays, n_samples)
    ok = np.ones(n_rays, bool)
    worst = {}
    for L in range(2):
        a, b = out[L], ref[L]
        ok &= (a["bin_idx"][:n_rays] == b["bin_idx"]).all(-1)
        for k in sorted(a):
            if k == "bin_idx" or k not in b:
                continue
            x = a[k][:n_rays].astype(np.float64)
            y = b[k].reshape(a[k][:n_rays].shape).astype(np.float64)
            lim = bar(k, y, {"grad_pred": b["grad_pred"].reshape(a["grad_pred"][:n_rays].shape)})
            if not k.startswith("r_") and k != "sdist":
                x, y, lim = x[ok], y[ok], lim[ok]
            assert np.isfinite(x).all(), (L, k)
            excess = np.abs(x - y) / lim
            worst[f"L{L}_{k}"] = (float(np.abs(x - y).max()), float(excess.max()))
    print(f"{batch} rays x {n_samples}, first {n_rays}: rays with the oracle's bin indices {int(ok.sum())};",
          "(largest |hip - oracle|, largest share of its bar):", {k: (f"{e:.2e}", f"{s:.2f}") for k, (e, s) in worst.items()})
    assert ok.sum() >= n_rays - 1, ok                    # (a tie at a CDF knot is one sample in ~1e5)
    assert np.array_equal(out[0]["sdist"][:n_rays], ref[0]["sdist"].reshape(out[0]["sdist"][:n_rays].shape))
    for k in PER_SAMPLE + ("r_rgb", "r_diffuse", "r_specular", "r_acc", "r_distance"):
        for L in range(2):
            assert f"L{L}_{k}" in worst, (L, k)
    for name, (err, share) in worst.items():
        assert share <= 1.0, (name, err, share)


def _bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("n_rays,n_samples,order", [(9, 128, "rotated"), (9, 128, "reversed"), (7, 72, "rotated")],
                         ids=["9x128_rotated", "9x128_reversed", "7x72_rotated"])
def test_placement_invariance_bitwise(hip, n_rays, n_samples, order):
    """the same rays rotated by one position / reversed: at 128 samples every ray lands on the other half of the waves of its
    pass or in another workgroup; at 72 samples a ray starts at sample 72 i of its workgroup, so rotating also moves it to
    the other 16-sample run and to other lanes.  After un-permuting, every output array is bit-equal per ray."""
    perm = np.roll(np.arange(n_rays), 1) if order == "rotated" else np.arange(n_rays)[::-1].copy()
    base = render(hip, np.arange(n_rays), n_samples, key=(n_rays, n_samples))
    moved = render(hip, perm, n_samples)
    inv = np.argsort(perm)                               # moved[inv[i]] is ray i
    bad = []
    for L in range(2):
        for k in sorted(base[L]):
            if not _bitwise(base[L][k], moved[L][k][inv]):
                x, y = base[L][k].astype(np.float64), moved[L][k][inv].astype(np.float64)
                bad.append((L, k, float(np.nanmax(np.abs(x - y)))))
        for k in PER_SAMPLE + ("r_rgb",):
            assert k in base[L], (L, k)
    print(f"{n_rays} rays x {n_samples} {order}: arrays that differ after un-permuting:", bad)
    assert not bad, bad
