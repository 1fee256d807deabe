"""GPU: the weight stream of the 16-bit eval kernels (`Pipe`, `issue_chunk` in csrc/refnerf_level_bf16.h) -- its position wraps at
the end of a pass, the split-f16 image rewinds behind the first spatial run, idle waves keep it going, and it stops after the
workgroup's last pass.  A wrong wrap or rewind feeds some layer the wrong weight chunk from that point on, so every case here
renders the SAME rays in batches that put them at different places of the stream (first / second pass of a workgroup, a full
or a partly filled pass, beside idle waves) and compares ray by ray.  The MLP of a sample depends on nothing but the sample,
and the per-ray phases run one ray per wave: where both renderings come from the same kernel the outputs are equal bit for
bit (asserted so; measured on the commit before the stream position became scalar and unchanged by it).  The ring variant
composites in another order than the plain kernel: its case says what is bitwise and what is held to a tolerance."""
import numpy as np
import pytest

from refnerf_pl_amd import synthetic
from test_hip_parity import DEV, O, hip, run_hip_model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BF16, F16X2 = 1, 3
RGB_TOL = 1e-4                                       # the parity bar of the f16x2 mode (tests/test_hip_f16x2.py)
KEYS = ("r_rgb", "weights", "sdist", "density")      # rendered colour, compositing weights, resampled distances, per-sample density
_BLOB = synthetic.make_params(seed=0, bias_scale=0.05, sharpen=20.0)
_RAYS = synthetic.blender_rays(2048, seed=21, center_frac=0.5)
_cache = {}


def render(hip, prec, n_rays, n_samples):
    """both levels of the first `n_rays` rays at `n_samples` per level (computed once per module)"""
    key = (prec, n_rays, n_samples)
    if key not in _cache:
        sub = {k: v[:n_rays] for k, v in _RAYS.items()}
        lv = dict(num_prop_samples=n_samples, num_nerf_samples=n_samples)
        _cache[key] = [{k: res[k] for k in KEYS} for res in run_hip_model(hip, _BLOB, sub, {}, lv, precision=prec)]
    return _cache[key]


def diffs(a, b, n):
    """per level and key: largest |a - b| over the first n rays, and whether they are the same bits"""
    out = {}
    for L in range(2):
        for k in KEYS:
            x, y = a[L][k][:n], b[L][k][:n]
            out[(L, k)] = (float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()), bool(np.array_equal(x.view(np.uint32), y.view(np.uint32))))
    return out


@pytest.mark.parametrize("prec", [F16X2, BF16], ids=["f16x2", "bf16"])
def test_small_batches_same_bits(hip, O, prec):
    """128 samples, two rays per workgroup (one 256-sample pass).  1 ray: a lone ray, waves 4-7 idle through the whole pass
    (`idle_pass` carries the stream, rewind included); 4 rays: full workgroups; 5 and 9 rays: full workgroups plus one with a
    half-filled pass.  Every ray must come out with the same bits in every batch that holds it; the f16x2 mode must also sit
    within 1e-4 RGB of the oracle on these rays."""
    sizes = (1, 4, 5, 9)
    outs = {n: render(hip, prec, n, 128) for n in sizes}
    for i, small in enumerate(sizes):
        for big in sizes[i + 1:]:
            d = diffs(outs[small], outs[big], small)
            print(f"prec {prec}: rays 0..{small - 1} alone vs in {big}:", {f"L{L}_{k}": v for (L, k), v in d.items()})
            for (L, k), (err, same) in d.items():
                assert same, (prec, small, big, L, k, err)
    if prec == F16X2:
        ref = O.model_forward(_BLOB, {k: v[:9] for k, v in _RAYS.items()}, num_prop_samples=128, num_nerf_samples=128)
        for n in sizes:
            for L in range(2):
                err = float(np.abs(outs[n][L]["r_rgb"] - ref[L]["r_rgb"][:n]).max())
                print(f"f16x2, {n} rays, level {L}: RGB L-inf vs oracle {err:.2e}")
                assert err <= RGB_TOL, (n, L, err)


def test_second_pass_same_bits(hip):
    """2048 rays x 128 samples is the smallest batch with FOUR rays per workgroup: two passes, the stream position wraps from
    the end of the image back to its start between them.  Rays 0-7 (first and second pass of two workgroups) against the same
    rays rendered in a batch of nine (one pass per workgroup): same kernel, same bits."""
    d = diffs(render(hip, F16X2, 9, 128), render(hip, F16X2, 2048, 128), 8)
    print("rays 0..7 in 9 vs in 2048 x 128:", {f"L{L}_{k}": v for (L, k), v in d.items()})
    for (L, k), (err, same) in d.items():
        assert same, (L, k, err)


def test_ring_variant_against_plain_kernel(hip):
    """2048 rays x 192 samples is the smallest batch that selects `level_fwd_f16x2_ring` (four rays = three full passes per
    workgroup, two wraps of the stream); the same eight rays alone take the plain kernel with one ray per workgroup (a partly
    filled pass, waves 6 and 7 idle).  Per-sample density, compositing weights and resampled distances are equal bit for bit.
    The rendered colour is NOT, and was not before the stream position became scalar: the ring variant composites a ray behind
    the pass that completes it, in another order of the sums (measured 2.4e-7 on both levels, on the commit before and after);
    it is held to the bar `test_record_ring_kernel` sets between the two variants, 2e-6."""
    d = diffs(render(hip, F16X2, 8, 192), render(hip, F16X2, 2048, 192), 8)
    print("rays 0..7 alone (plain kernel) vs in 2048 x 192 (ring variant):", {f"L{L}_{k}": v for (L, k), v in d.items()})
    for (L, k), (err, same) in d.items():
        if k == "r_rgb":
            assert err <= 2e-6, (L, k, err)
        else:
            assert same, (L, k, err)
