"""Guard bands: a guarded allocator for the tensors a library entry reads and fills.

Every output the library fills is normally a `torch.empty` block of the caching allocator, which rounds sizes up and
recycles blocks: a store a few elements outside an output lands in slack, an element a kernel skips may still hold the
right number from the previous call.  `Arena.alloc` instead places a tensor in the middle of a buffer of its own,

    [ red zone | payload | red zone ]

fills the red zones with one word pattern and an output's payload with a sentinel word, and `Arena.check` asserts that
no red-zone byte changed, that no input changed and that no 32-bit word of a "fully written" output still holds the
sentinel.  `guarded(arena)` routes the allocations of the `_hip` wrappers through an arena.  Plain helper module
(like helpers.py); tests/test_guards_cpu.py proves on CPU tensors that each kind of planted error is reported.
"""
import contextlib
import sys

import numpy as np
import torch

SENTINEL_WORD = 0x7FA55AA5       # payload of an output: a NaN with a payload of its own as float32, 2141543077 as an index
REDZONE_WORD = 0xA5A5A5A5        # red zones of outputs and workspaces (-5.7e-16 as float32, negative as an index)
MIN_ZONE = 4096
MAX_ZONE = 4 << 20
ALIGN = 512                      # what the caching allocator gives production tensors


def _round_up(n, m):
    return (n + m - 1) // m * m


def zone_bytes(shape, itemsize):
    """Red-zone length per side: max(4 KiB, 8 rows of the leading dimension, the tensor's own size), rounded up to 512,
    capped at 4 MiB -- a tail workgroup that writes whole rows past the end must still land inside it."""
    nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize if len(shape) else itemsize
    row = nbytes // max(int(shape[0]), 1) if len(shape) else nbytes
    return min(_round_up(max(MIN_ZONE, 8 * row, nbytes), ALIGN), MAX_ZONE)


def _word_bytes(word):
    return np.array([word], dtype="<u4").view(np.uint8)


def _value_bytes(value, dtype):
    """the 8 bytes that repeat through a red zone holding `value` of `dtype` (1, 2, 4 or 8 bytes wide)"""
    b = torch.full((1,), value, dtype=dtype).view(torch.uint8).numpy()
    return np.tile(b, 8 // len(b))


class _Record:
    __slots__ = ("name", "buf", "lead", "nbytes", "zone", "pattern", "view", "written", "reason", "snapshot")


class Arena:
    """One guarded call's tensors.  float_zone: what the red zones of float inputs hold (0.0 or nan in the tests); the
    red zones of integer inputs hold the in-range value the caller names; outputs and workspaces REDZONE_WORD."""

    def __init__(self, device="cpu", float_zone=0.0):
        self.device = torch.device(device)
        self.float_zone = float_zone
        self.records = []
        self._expected = {}

    # the arena's own allocations must not come back through an interposed torch.empty
    _empty = staticmethod(torch.empty)

    def _pattern(self, pattern, nbytes, device):
        key = (pattern.tobytes(), nbytes, str(device))
        if key not in self._expected:
            self._expected[key] = torch.from_numpy(np.tile(pattern, nbytes // len(pattern))).to(device)
        return self._expected[key]

    def _place(self, shape, dtype, device, zone_pattern, name):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        device = self.device if device is None else torch.device(device)
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        zone = zone_bytes(shape, itemsize)
        r = _Record()
        r.name = name or f"tensor{len(self.records)}"
        r.buf = Arena._empty(zone + nbytes + zone, dtype=torch.uint8, device=device)
        assert r.buf.data_ptr() % itemsize == 0
        r.lead, r.nbytes, r.zone, r.pattern = zone, nbytes, zone, zone_pattern
        expected = self._pattern(zone_pattern, zone, device)
        r.buf[:zone].copy_(expected)
        r.buf[zone + nbytes:].copy_(expected)       # the trailing zone starts at the first byte after the payload
        r.view = r.buf[zone:zone + nbytes].view(dtype).view(shape)
        r.written, r.reason, r.snapshot = False, None, None
        self.records.append(r)
        return r

    def alloc(self, shape, dtype=torch.float32, device=None, fill="sentinel", name=None, reason=None):
        """A contiguous tensor between two red zones.  fill = "sentinel": an output every element of which the entry must
        write (payload = SENTINEL_WORD, checked); fill = None with a `reason` naming the header line: an output the header
        documents as accumulated into, optional or scratch -- red zones only; fill = a number: red zones only, that content."""
        r = self._place(shape, dtype, device, _word_bytes(REDZONE_WORD), name)
        if isinstance(fill, str):
            assert fill == "sentinel", fill
            words = r.nbytes // 4
            r.buf[r.lead:r.lead + 4 * words].copy_(self._pattern(_word_bytes(SENTINEL_WORD), 4 * words, r.buf.device))
            if r.nbytes % 4:    # (a byte tensor's odd tail)
                r.buf[r.lead + 4 * words:r.lead + r.nbytes].copy_(self._pattern(_word_bytes(SENTINEL_WORD), 4, r.buf.device)[:r.nbytes % 4])
            r.written = True
        else:
            r.reason = reason or "caller-filled"
            if fill is not None:
                r.view.fill_(fill)
        return r.view

    def put(self, t, name=None, int_zone=None, inout=None):
        """A guarded copy of the input `t`.  Red zones: self.float_zone for float tensors, `int_zone` (an in-range value, the
        same in every run) for integer ones.  check() also asserts the payload unchanged, unless `inout` (a reason) says
        the entry updates it in place."""
        if t.dtype.is_floating_point:
            pattern = _value_bytes(self.float_zone, t.dtype)
        elif t.dtype == torch.uint8 and int_zone is None:
            pattern = _value_bytes(0, t.dtype)
        else:
            assert int_zone is not None, "integer inputs name the in-range value their red zones hold"
            pattern = _value_bytes(int_zone, t.dtype)
        r = self._place(t.shape, t.dtype, t.device, pattern, name)
        r.view.copy_(t)
        r.reason = inout or "input"
        if inout is None:
            r.snapshot = r.buf[r.lead:r.lead + r.nbytes].clone()
        return r.view

    def _record_of(self, t):
        for r in self.records:
            if r.view.data_ptr() == t.data_ptr() and r.nbytes == t.numel() * t.element_size():
                return r
        raise KeyError("not a tensor of this arena")

    def owns(self, t):
        try:
            self._record_of(t)
            return True
        except KeyError:
            return False

    def holds(self, t):
        """True when `t` lives in one of the arena's buffers: a tensor it handed out, or a view of one"""
        base = t.untyped_storage().data_ptr()
        return any(r.buf.untyped_storage().data_ptr() == base for r in self.records)

    def loose(self, t, reason):
        """Register the output `t` as "red zones only": `reason` names the header line that says it is accumulated into,
        optional or scratch."""
        r = self._record_of(t)
        r.written, r.reason = False, reason

    def rename(self, t, name):
        self._record_of(t).name = name

    def check(self):
        """Assert: every red-zone byte unchanged (tensor, side, first and last changed offset), every input unchanged, and
        no aligned 32-bit word of a fully written output still the sentinel (first flat index, count)."""
        problems = []
        flags = []
        for r in self.records:
            expected = self._pattern(r.pattern, r.zone, r.buf.device)
            f = [(r.buf[:r.lead] != expected).any(), (r.buf[r.lead + r.nbytes:] != expected).any()]
            if r.snapshot is not None:
                f.append((r.buf[r.lead:r.lead + r.nbytes] != r.snapshot).any())
            if r.written and r.nbytes >= 4:
                f.append((r.buf[r.lead:r.lead + r.nbytes // 4 * 4].view(torch.int32) == _sentinel_i32()).any())
            flags.append(torch.stack(f).any())
        if not flags or not bool(torch.stack([f.to(self.device) for f in flags]).any()):      # one synchronisation
            return
        for r in self.records:        # the slow path: something tripped
            expected = self._pattern(r.pattern, r.zone, r.buf.device)
            for side, zone in (("leading", r.buf[:r.lead]), ("trailing", r.buf[r.lead + r.nbytes:])):
                bad = (zone != expected).nonzero().reshape(-1)
                if bad.numel():
                    first, last = int(bad[0]), int(bad[-1])
                    if side == "leading":      # offsets relative to the payload: negative = before its first byte
                        first, last = first - r.lead, last - r.lead
                        where = f"bytes {first} .. {last} before the payload's start"
                    else:
                        where = f"bytes {first} .. {last} past the payload's end"
                    problems.append(f"{r.name}: {side} red zone overwritten, {bad.numel()} bytes changed, {where} "
                                    f"(payload {tuple(r.view.shape)} {r.view.dtype}, {r.nbytes} bytes)")
            if r.snapshot is not None:
                bad = (r.buf[r.lead:r.lead + r.nbytes] != r.snapshot).nonzero().reshape(-1)
                if bad.numel():
                    problems.append(f"{r.name}: input modified, {bad.numel()} bytes changed, first at byte {int(bad[0])}, last at {int(bad[-1])}")
            if r.written and r.nbytes >= 4:
                words = r.buf[r.lead:r.lead + r.nbytes // 4 * 4].view(torch.int32)
                bad = (words == _sentinel_i32()).nonzero().reshape(-1)
                if bad.numel():
                    per = max(r.view.element_size() // 4, 1)
                    problems.append(f"{r.name}: {bad.numel()} 32-bit words never written, first at flat index {int(bad[0]) // per} "
                                    f"(payload {tuple(r.view.shape)} {r.view.dtype})")
        assert not problems, "guard bands:\n  " + "\n  ".join(problems)


def _sentinel_i32():
    return int(np.array([SENTINEL_WORD], dtype="<u4").view("<i4")[0])


SENTINEL_I32 = _sentinel_i32()


def _shape_of(args, kwargs):
    if "size" in kwargs:
        return kwargs["size"]
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(args[0])
    return tuple(args)


@contextlib.contextmanager
def guarded(arena, hip=None, modules=("refnerf_pl_amd._hip",)):
    """Route the allocations of the `_hip` wrappers through `arena`: for the duration torch.empty gives sentinel-filled,
    fully checked outputs (byte tensors -- the wrappers' workspaces and the activation buffer -- red zones only), and
    torch.zeros / torch.full red-zone-only tensors with their real contents.  Only calls made from `modules` are routed;
    everything else, the arena itself included, keeps the original allocator.  `hip`: the _hip module, whose cached
    backward workspace is set aside for the scope so that it is allocated under guard too."""
    orig = {name: getattr(torch, name) for name in ("empty", "zeros", "full")}

    def routed(name):
        def alloc(*args, **kwargs):
            caller = sys._getframe(1)
            if caller.f_globals.get("__name__") not in modules or kwargs.get("out") is not None:
                return orig[name](*args, **kwargs)
            where = f"{caller.f_code.co_name}:{caller.f_lineno}"
            dtype = kwargs.get("dtype") or torch.get_default_dtype()
            device = kwargs.get("device")
            if name == "full":
                shape, value = (kwargs["size"] if "size" in kwargs else args[0]), (kwargs["fill_value"] if "fill_value" in kwargs else args[1])
                if kwargs.get("dtype") is None:
                    dtype = torch.get_default_dtype() if isinstance(value, float) else torch.int64
                return arena.alloc(shape, dtype, device, fill=value, name=where, reason="torch.full of the wrapper: caller-initialised")
            shape = _shape_of(args, kwargs)
            if name == "zeros":
                return arena.alloc(shape, dtype, device, fill=0, name=where, reason="torch.zeros of the wrapper: caller-initialised")
            if dtype == torch.uint8:
                return arena.alloc(shape, dtype, device, fill=None, name=where,
                                   reason="byte buffers of the wrappers are workspaces (refnerf_hip.h: d_workspace / d_activations, opaque to the caller)")
            return arena.alloc(shape, dtype, device, fill="sentinel", name=where)
        return alloc

    saved_ws = None
    if hip is not None:
        saved_ws = dict(hip._workspace)
        hip._workspace.clear()
    try:
        for name in orig:
            setattr(torch, name, routed(name))
        yield arena
    finally:
        for name, fn in orig.items():
            setattr(torch, name, fn)
        if hip is not None:
            hip._workspace.clear()
            hip._workspace.update(saved_ws)
