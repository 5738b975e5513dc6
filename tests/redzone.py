"""Red zones around every device buffer the C ABI touches (a plain helper module: no fixture, no conftest).

`with guarded() as rz:` replaces, for its duration and in eager mode only,

* ``lib.call``: for every call the distinct underlying STORAGES of all tensor arguments are collected (storage, not view,
  granularity: aliased arguments stay aliased, and a `ptr, ld, coff` argument that addresses a wider tensor than the view it
  was taken from stays valid).  Per storage a fresh arena ``[guard | exact storage bytes | guard]`` is built, the storage copied
  in, ``arena + guard + (t.data_ptr() - storage.data_ptr())`` passed in place of the tensor, the entry point run, the bytes
  copied back and both guards compared byte for byte with their fill -- all enqueued on the current stream; one read of a flag
  ends the call.  The guard is ``max(1 MiB, storage bytes)`` capped at 8 MiB, rounded up to 512 bytes so that the substituted
  address keeps the alignment (mod 512) the caching allocator gave the original.  Damage raises `GuardDamage` with the entry
  point, the argument positions that address the storage and the byte range of the first damaged run relative to the buffer's
  end (trailing guard) or start (leading guard).
* ``ops.scratch``: a fresh tensor of exactly the requested bytes (rounded up to whole floats only), no reuse, no 1024-float
  floor, prefilled with poison.  A request of zero bytes still gets a guarded, non-NULL address: the arena of an empty storage
  is ``[guard | guard]``.
* ``ops.new`` / ``ops._i16``: poison-filled outright.

Poison: 0xFF bytes for floating-point and int16 storages (int16 holds packed fp16 here) -- both read as NaN, so an over-read or a
never-written element that reaches a result shows as non-finite -- and 0x00 for uint8 / int32 / int64 storages (labels, offset
and descriptor tables): a poison value is never something a kernel could use as an index.  Guards carry the poison of their
storage, so an over-READ is harmless and visible; a store of the fill value itself into a guard is the one thing the byte
comparison cannot see.

`poison_allocator()` releases the caching allocator's free blocks and leaves a few hundred MB of 0xFF-filled blocks in their
place, so that the `torch.empty*` sites start from NaN instead of from the previous run's answer; an arena is re-poisoned before
it goes back to the allocator for the same reason.

Pass-through: a pointer argument that cannot be guarded -- a raw ``int`` / ``c_void_p`` address, or device pointers held inside
a descriptor table or a host struct -- is counted and allowed only for the entry points of `ALLOWLIST`; anywhere else it raises
`PassThrough`.  Host structs themselves (``ctypes.byref(geom)``) are not device memory and are not counted.

The arena logic is device-agnostic: `RedZone(invoke=...)` takes any callable as "the entry points" (tests/test_redzone_host.py
runs it on CPU tensors with stand-ins that misbehave inside their arena).

Access patterns the harness models on purpose:
* an argument of zero elements is still given an address (see above) -- the library never dereferences it;
* the same storage may be passed several times at different offsets (views of one flat buffer): one arena, one copy.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

GUARD_MIN = 1 << 20
GUARD_CAP = 8 << 20
_NAN_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.int16)

# entry point -> why some of its pointers cannot be put in an arena
ALLOWLIST = {
    "image_to_u8": "destination is a visuals.Window: a raw address into the caller's uint8 canvas",
    "label_colorize": "destination is a visuals.Window: a raw address into the caller's uint8 canvas",
    "bilinear_up_u8": "source and destination are visuals.Windows: raw addresses into uint8 canvases",
    "bicubic_up": "destination may be a visuals.Window: a raw address into the caller's uint8 canvas",
    "grad_gather": "grad_ptrs is a device table of the addresses of the autograd gradients (FlatAdam)",
    "spectral_norm_group_fwd": "the dsee_sn_layer table holds the device addresses of w_orig / u / v of every layer",
    "spade_resblock_fwd": "dsee_norm_layer is a host struct of device pointers",
    "spade_resblock_train_fwd": "dsee_norm_layer / dsee_block_noise are host structs of device pointers",
    "spade_resblock_bwd": "dsee_norm_layer / dsee_block_noise / dsee_block_grads are host structs of device pointers",
}
# entry points whose tensor or struct arguments hold further device pointers: one pass-through counted per call
DESCRIPTOR_TABLES = {"grad_gather", "spectral_norm_group_fwd", "spade_resblock_fwd", "spade_resblock_train_fwd",
                     "spade_resblock_bwd"}


class GuardDamage(AssertionError):
    def __init__(self, entry, argpos, side, lo, hi):
        self.entry, self.argpos, self.side, self.lo, self.hi = entry, tuple(argpos), side, lo, hi
        where = ("bytes [+%d, +%d) past the end" % (lo, hi)) if side == "end" else \
                ("bytes [-%d, -%d) before the start" % (lo, hi))
        super().__init__("dsee_%s wrote outside the buffer of argument %s: %s" % (entry, list(argpos), where))


class PoisonLeak(AssertionError):
    def __init__(self, entry, argpos, offset):
        self.entry, self.argpos, self.offset = entry, tuple(argpos), offset
        super().__init__("dsee_%s left a non-finite value at byte %d of the buffer of argument %s, whose contents were finite "
                         "before the call: poison read from a workspace / output element nobody wrote, or from a guard"
                         % (entry, offset, list(argpos)))


class PassThrough(AssertionError):
    pass


def poison_of(dtype):
    return 0xFF if dtype in _NAN_DTYPES else 0x00


def guard_bytes(nbytes, lo=GUARD_MIN, cap=GUARD_CAP):
    return (min(max(lo, nbytes), cap) + 511) // 512 * 512


def _bytes_of(storage, device):
    return torch.empty(0, dtype=torch.uint8, device=device).set_(storage, 0, (storage.nbytes(),))


def _first_run(guard_cpu, fill):
    """[lo, hi) of the first run of bytes that differ from `fill`."""
    bad = np.flatnonzero(guard_cpu.numpy() != fill)
    lo = int(bad[0])
    hi = lo + 1
    later = set(bad[1:65536].tolist())
    while hi in later:
        hi += 1
    return lo, hi


class RedZone:
    """invoke(name, *args): the entry points; called with every tensor argument replaced by the int address inside its arena."""

    def __init__(self, invoke, protos=None, allow=ALLOWLIST, descriptor_tables=DESCRIPTOR_TABLES, device="cuda",
                 guard_min=GUARD_MIN, guard_cap=GUARD_CAP, nan_watch=False):
        self.invoke, self.protos, self.allow, self.tables = invoke, protos, allow, descriptor_tables
        self.device, self.guard_min, self.guard_cap, self.nan_watch = device, guard_min, guard_cap, nan_watch
        self.calls = 0            # calls substituted
        self.passthrough = {}     # entry -> pointer arguments passed through unguarded
        self.guarded = set()      # entry points that ran with at least one storage in an arena

    # -------------------------------------------------------------------------------------------- lib.call
    def _raw_pointers(self, name, args):
        n = 1 if name in self.tables else 0
        argtypes = None if self.protos is None else self.protos.get("dsee_" + name, (None, None))[1]
        for i, a in enumerate(args):
            if isinstance(a, C.c_void_p):
                a = a.value or 0
            if isinstance(a, bool) or not isinstance(a, int) or a == 0:
                continue
            if argtypes is not None and i < len(argtypes) and argtypes[i] is C.c_void_p:
                n += 1
        return n

    def call(self, name, *args):
        raw = self._raw_pointers(name, args)
        if raw:
            if name not in self.allow:
                raise PassThrough("dsee_%s: %d pointer argument(s) cannot be guarded and the entry point is not in "
                                  "redzone.ALLOWLIST" % (name, raw))
            self.passthrough[name] = self.passthrough.get(name, 0) + raw
        groups = {}               # storage key -> [storage, dtype, positions]
        for i, a in enumerate(args):
            if not isinstance(a, torch.Tensor):
                continue
            assert a.is_contiguous() and a.device.type == torch.device(self.device).type, \
                "dsee_%s argument %d: device-resident contiguous tensor required" % (name, i)
            st = a.untyped_storage()
            key = st.data_ptr() if st.nbytes() else ("empty", id(a))
            groups.setdefault(key, [st, a.dtype, []])[2].append(i)
        if not groups:
            return self.invoke(name, *args)
        new_args = list(args)
        arenas = []
        for st, dtype, pos in groups.values():
            n, fill = st.nbytes(), poison_of(dtype)
            g = guard_bytes(n, self.guard_min, self.guard_cap)
            arena = torch.empty(2 * g + n, dtype=torch.uint8, device=self.device)
            arena[:g].fill_(fill)
            arena[g + n:].fill_(fill)
            body = _bytes_of(st, self.device) if n else None
            clean = None
            if n:
                arena[g:g + n].copy_(body)
                if self.nan_watch and dtype == torch.float32 and n % 4 == 0:
                    clean = torch.isfinite(body.view(torch.float32)).all()
            for i in pos:
                new_args[i] = arena.data_ptr() + g + (args[i].data_ptr() - st.data_ptr() if n else 0)
            arenas.append((arena, body, g, n, fill, pos, clean))
        self.invoke(name, *new_args)
        self.calls += 1
        self.guarded.add(name)
        flags = []
        for arena, body, g, n, fill, pos, clean in arenas:
            if n:
                body.copy_(arena[g:g + n])
            flags.append((arena[:g] != fill).any())
            flags.append((arena[g + n:] != fill).any())
            flags.append(clean & ~torch.isfinite(body.view(torch.float32)).all() if clean is not None
                         else torch.zeros((), dtype=torch.bool, device=self.device))
        hit = torch.stack(flags).cpu().tolist()         # the one synchronising read of the call
        for k, (arena, body, g, n, fill, pos, clean) in enumerate(arenas):
            if hit[3 * k]:
                lo, hi = _first_run(arena[:g].cpu(), fill)
                raise GuardDamage(name, pos, "start", g - lo, g - hi)
            if hit[3 * k + 1]:
                lo, hi = _first_run(arena[g + n:].cpu(), fill)
                raise GuardDamage(name, pos, "end", lo, hi)
            if hit[3 * k + 2]:
                bad = (~torch.isfinite(body.view(torch.float32))).nonzero()[0]
                raise PoisonLeak(name, pos, int(bad) * 4)
            if n:
                arena[g:g + n].fill_(fill)              # the block returns to the allocator poisoned, not holding the answer

    # -------------------------------------------------------------------------------------------- ops.scratch / new / _i16
    def scratch(self, nbytes, tag="ws"):
        n = (int(nbytes) + 3) // 4
        t = torch.empty(n, dtype=torch.float32, device=self.device)
        if n:
            t.view(torch.uint8).fill_(0xFF)
        return t

    def new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device).fill_(float("nan"))

    def i16(self, n):
        return torch.empty(n, dtype=torch.int16, device=self.device).fill_(-1)


def poison_allocator(total_mb=384):
    """Release the caching allocator's free blocks, then leave 0xFF-filled blocks of assorted sizes in their place."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    sizes = [1 << 10, 16 << 10, 256 << 10, 1 << 20, 4 << 20, 16 << 20, 64 << 20]
    share = (total_mb << 20) // len(sizes)
    held = []
    for s in sizes:
        for _ in range(max(1, min(64, share // s))):
            held.append(torch.full((s,), 0xFF, dtype=torch.uint8, device="cuda"))
    del held
    torch.cuda.synchronize()


# what every guarded() block of this process has seen (tests/test_gpu_redzone.py's coverage condition reads it)
RECORD = {"calls": 0, "passthrough": {}, "guarded": set(), "scenarios": 0}


@contextlib.contextmanager
def guarded(poison=True, **kw):
    """Run the body with lib.call, ops.scratch, ops.new and ops._i16 replaced as the module docstring says."""
    from deepsee_amd import lib as L, ops
    assert not torch.cuda.is_current_stream_capturing(), "eager mode only"
    if poison:
        poison_allocator()
    rz = RedZone(L.call, protos=L.header_prototypes(), **kw)
    saved = (L.call, ops.scratch, ops.new, ops._i16)
    L.call, ops.scratch, ops.new, ops._i16 = rz.call, rz.scratch, rz.new, rz.i16
    try:
        yield rz
        torch.cuda.synchronize()
    finally:
        L.call, ops.scratch, ops.new, ops._i16 = saved
        RECORD["calls"] += rz.calls
        RECORD["guarded"] |= rz.guarded
        RECORD["scenarios"] += 1
        for k, v in rz.passthrough.items():
            RECORD["passthrough"][k] = RECORD["passthrough"].get(k, 0) + v
