"""The weight packers (csrc/refnerf_pack.h), per image kind, on the seeded blob:
    python scripts/time_pack.py                          # the in-tree library
    REFNERF_LIB=ab/x.so python scripts/time_pack.py      # an A/B build
10 warm-up packs, then 20 windows of 100 back-to-back packs with one HIP-event pair per window; median and p10 - p90 of the
windows in us per pack; one JSON line at the end.  The entries are called through ctypes with their arguments prepared once, so
that a window holds launches and nothing else.  f16x2_train (pack_train_chunks + pack_train_consts) is the one that runs in every
training step; f32-G7 is refnerf_pack_weights_basis with the 21 directions of icosahedron / 2.
An A/B comparison runs this as alternating child processes (A B A B): the gap between A's two medians is the noise figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import refnerf_pl_amd  # noqa: E402,F401
from refnerf_pl_amd import _hip, geopoly, synthetic  # noqa: E402

WINDOWS, PER, WARM = 20, 100, 10
KINDS = (("f32", _hip.PREC_F32, 0), ("bf16", _hip.PREC_BF16, 0), ("f16", _hip.PREC_F16, 0), ("f16x2", _hip.PREC_F16X2, 0),
         ("f16x2_train", _hip.IMAGE_F16X2_TRAIN, 0), ("f32-G7", _hip.PREC_F32, 7))


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(WINDOWS)]
    for a, b in ev:
        a.record()
        for _ in range(PER):
            fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 / PER for a, b in ev])
    return dict(median_us=float(np.median(us)), p10_us=float(np.percentile(us, 10)), p90_us=float(np.percentile(us, 90)))


def main():
    _hip.require_device()
    lib, st = _hip.lib(), _hip.stream_ptr()
    out = dict(lib=_hip.LIB_PATH)
    for name, kind, groups in KINDS:
        if groups > 1:
            P = torch.from_numpy(synthetic.make_basis_params(n_basis=3 * groups, seed=0)).to("cuda:0")
            basis = torch.from_numpy(np.ascontiguousarray(geopoly.generate_basis("icosahedron", 2), np.float32)).to("cuda:0")
        else:
            P, basis = torch.from_numpy(synthetic.make_params(seed=0)).to("cuda:0"), None
        img = _hip.pack_weights(P, precision=kind, basis=basis)
        if groups > 1:
            def fn(a=(_hip.ptr(P), _hip.ptr(basis), groups, _hip.ptr(img), kind, st)):
                _hip.check(lib.refnerf_pack_weights_basis(*a))
        else:
            def fn(a=(_hip.ptr(P), _hip.ptr(img), kind, st)):
                _hip.check(lib.refnerf_pack_weights(*a))
        out[name] = timed(fn)
        print(name, {k: round(v, 2) for k, v in out[name].items()}, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
