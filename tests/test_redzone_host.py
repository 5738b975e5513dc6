"""The red-zone harness (tests/redzone.py) on CPU tensors: the "entry points" are stand-ins that misbehave INSIDE their arena
(ctypes.memmove on the substituted addresses), so every report is checked without any kernel doing wrong."""
import ctypes as C
import struct

import pytest
import torch

import redzone as R

ONE = struct.pack("f", 1.0)


def put(addr, values):
    buf = struct.pack("%df" % len(values), *values)
    C.memmove(addr, buf, len(buf))


def get(addr, n):
    buf = C.create_string_buffer(4 * n)
    C.memmove(buf, addr, 4 * n)
    return list(struct.unpack("%df" % n, buf.raw))


def harness(standins, **kw):
    """standins: name -> (callable, signature), signature one letter per argument: p = pointer, i = scalar"""
    def invoke(name, *args):
        return standins[name][0](*args)
    protos = {"dsee_" + k: (C.c_int, [C.c_void_p if c == "p" else C.c_long for c in sig]) for k, (_, sig) in standins.items()}
    return R.RedZone(invoke, protos=protos, device="cpu", **kw)


def test_guard_size_rule():
    assert R.guard_bytes(16) == 1 << 20 and R.guard_bytes(3 << 20) == 3 << 20 and R.guard_bytes(1 << 30) == 8 << 20
    assert R.guard_bytes((1 << 20) + 4) == (1 << 20) + 512          # alignment of the substituted address is kept
    assert R.poison_of(torch.float32) == 0xFF and R.poison_of(torch.int16) == 0xFF
    assert [R.poison_of(d) for d in (torch.uint8, torch.int32, torch.int64)] == [0, 0, 0]


def test_write_one_float_past_the_end_is_reported():
    def over(n, x, y, count):
        put(y, [2.0] * count + [1.0])          # count floats of y, and one more
    rz = harness({"over": (over, "ippi")})
    x, y = torch.zeros(5), torch.zeros(7)
    with pytest.raises(R.GuardDamage) as e:
        rz.call("over", 3, x, y, 7)
    assert (e.value.entry, e.value.argpos, e.value.side, e.value.lo, e.value.hi) == ("over", (2,), "end", 0, 4)
    assert "dsee_over" in str(e.value) and "[+0, +4) past the end" in str(e.value)
    assert y.tolist() == [2.0] * 7              # what it wrote inside came back all the same


def test_write_past_the_end_of_a_view_is_measured_from_the_storage():
    """Storage granularity: a view's own end is not a boundary, the storage's is."""
    def over(y, count):
        put(y + 4 * count, [1.0])
    rz = harness({"over": (over, "pi")})
    base = torch.zeros(16)
    rz.call("over", base[4:8], 4)               # lands in base[8]: inside the storage, a legitimate `ptr, ld` access
    assert base[8] == 1.0
    with pytest.raises(R.GuardDamage) as e:
        rz.call("over", base[12:], 6)           # two floats past the storage
    assert (e.value.argpos, e.value.side, e.value.lo, e.value.hi) == ((0,), "end", 8, 12)


def test_write_one_float_before_the_start_is_reported():
    def under(x, y):
        put(y - 4, [1.0])
    rz = harness({"under": (under, "pp")})
    x, y = torch.zeros(5), torch.zeros(7)
    with pytest.raises(R.GuardDamage) as e:
        rz.call("under", x, y)
    assert (e.value.entry, e.value.argpos, e.value.side, e.value.lo, e.value.hi) == ("under", (1,), "start", 4, 0)
    assert "[-4, -0) before the start" in str(e.value)


def test_zero_written_past_an_index_table_is_not_confused_with_its_guard_but_a_one_is():
    def over(t, n):
        C.memmove(t + 4 * n, struct.pack("i", 7), 4)
    rz = harness({"over": (over, "pi")})
    with pytest.raises(R.GuardDamage) as e:
        rz.call("over", torch.zeros(6, dtype=torch.int32), 6)
    assert (e.value.side, e.value.lo, e.value.hi) == ("end", 0, 1)      # 07 00 00 00: one byte differs from the 0x00 fill


def test_unwritten_poisoned_scratch_summed_into_the_output_is_reported():
    def reduce(x, ws, n_ws, out):
        put(ws, get(x, n_ws - 1))                          # leaves the last workspace element unwritten
        put(out, [sum(get(ws, n_ws))])
    rz = harness({"reduce": (reduce, "ppip")}, nan_watch=True)
    ws = rz.scratch(4 * 6)
    assert ws.numel() == 6 and ws.dtype == torch.float32 and bool(torch.isnan(ws).all())
    assert rz.scratch(5).numel() == 2 and rz.scratch(0).numel() == 0          # whole floats, no floor
    assert rz.scratch(24).data_ptr() != ws.data_ptr()                         # no reuse
    x, out = torch.ones(8), torch.zeros(3)
    with pytest.raises(R.PoisonLeak) as e:
        rz.call("reduce", x, ws, 6, out)
    assert (e.value.entry, e.value.argpos, e.value.offset) == ("reduce", (3,), 0)
    assert "dsee_reduce" in str(e.value)
    # the same stand-in with the workspace size it really needs is clean
    rz.call("reduce", x, rz.scratch(4 * 6), 7 - 1, out)


def test_over_read_of_a_guard_shows_as_nan():
    def read_past(x, n, out):
        put(out, [sum(get(x, n + 1))])
    rz = harness({"read_past": (read_past, "pip")})
    x, out = torch.ones(4), torch.zeros(1)
    rz.call("read_past", x, 4, out)                        # a read damages nothing ...
    assert bool(torch.isnan(out).all())                    # ... and what it read was poison


def test_aliased_views_of_one_storage_share_one_arena():
    seen = {}

    def axpy(a, b, n):
        seen["delta"] = b - a
        put(b, [2 * v for v in get(a, n)])
        put(a, [v + 1 for v in get(a, n)])
    rz = harness({"axpy": (axpy, "ppi")})
    flat = torch.arange(8, dtype=torch.float32)
    lo, hi = flat[:4], flat[4:]
    rz.call("axpy", lo, hi, 4)
    assert seen["delta"] == 16                             # still 4 floats apart: one arena
    assert flat.tolist() == [1, 2, 3, 4, 0, 2, 4, 6] and (rz.calls, rz.guarded, rz.passthrough) == (1, {"axpy"}, {})


def test_raw_addresses_pass_only_for_allowlisted_entry_points():
    def touch(dst, n):
        put(dst, [5.0] * n)
    t = torch.zeros(4)
    rz = harness({"touch": (touch, "pi"), "window": (touch, "pi")}, allow={"window": "a raw address into the caller's canvas"},
                 descriptor_tables=())
    with pytest.raises(R.PassThrough, match="dsee_touch"):
        rz.call("touch", t.data_ptr(), 4)
    rz.call("window", C.c_void_p(t.data_ptr()), 4)
    assert t.tolist() == [5.0] * 4 and rz.passthrough == {"window": 1} and rz.guarded == set()
    rz.call("touch", None, 0)                              # NULL and host structs are not device pointers
    rz.call("touch", C.byref(C.c_int(0)), 0)
    assert rz.passthrough == {"window": 1}


def test_every_descriptor_table_entry_point_is_allowlisted_with_a_reason():
    assert set(R.DESCRIPTOR_TABLES) <= set(R.ALLOWLIST) and all(len(v) > 10 for v in R.ALLOWLIST.values())
