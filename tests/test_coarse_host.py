"""The coarse entry points (deepsee_amd/csrc/coarse.cpp) on the host: the three block entry points share one argument check, and
the caller-owned workspaces and the saved area are no larger than before the file laid all of them out with one arena.  Nothing
here launches a kernel: device pointers are the address 4096 and are never dereferenced, the norm structs are host buffers.

tests/golden/coarse_workspace.json holds the byte counts of the commit before the one-arena layout, written there by
`python tests/test_coarse_host.py > tests/golden/coarse_workspace.json`."""
import ctypes
import json
import os

SHAPES = [(8, 256, 256, 512), (8, 64, 64, 512), (4, 128, 128, 256), (4, 64, 64, 1024), (2, 32, 32, 64)]
INFERENCE = ("dsee_sean_norm_fwd_workspace", "dsee_spade_resblock_fwd_workspace")
TRAINING = ("dsee_spade_resblock_saved_bytes", "dsee_spade_resblock_train_fwd_workspace", "dsee_spade_resblock_bwd_workspace")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coarse_workspace.json")


def _sizes():
    """{function: {"N,H,W,C,label_nc,has_table": bytes}}: every size function at every shape it is asked at (the last shape is
    below what the training pair tiles: norm forward and inference block only)."""
    from deepsee_amd import lib as L
    so = L.lib()
    out = {}
    for fn in INFERENCE + TRAINING:
        for shape in SHAPES if fn in INFERENCE else SHAPES[:-1]:
            for nc in (1, 19, 32):
                for has_t in (0, 1):
                    args = (*shape, nc, has_t)
                    extra = (shape[1], shape[2], 0) if fn == "dsee_spade_resblock_bwd_workspace" else ()    # lab_h, lab_w, shift
                    out.setdefault(fn, {})[",".join(map(str, args))] = getattr(so, fn)(*args, *extra)
    return out


def test_workspace_and_saved_sizes_do_not_grow():
    parent = json.load(open(GOLDEN))
    got = _sizes()
    assert set(got) == set(parent) == set(INFERENCE + TRAINING)
    for fn, sizes in got.items():
        assert set(sizes) == set(parent[fn]) and len(sizes) == (30 if fn in INFERENCE else 24), fn
        for key, nbytes in sizes.items():
            print(fn, key, nbytes, parent[fn][key])
            assert 0 < nbytes <= parent[fn][key], (fn, key, nbytes, parent[fn][key])


def _block_calls(so, n0, n1, lab, shift, nc=19, N=4, R=128, Cc=256):
    """The three block entry points on the same two norm structs, label map and shape; {name: (return code, error text)}."""
    one = ctypes.c_void_p(4096)                       # non-null, never dereferenced
    big = 1 << 40
    out = {}
    rc = so.dsee_spade_resblock_bwd(n0, one, n1, one, None, one, lab, lab, shift, nc, one, one, one, n0, one, one, 0.2, N, R, R, Cc,
                                    one, big, one, big, None)
    out["dsee_spade_resblock_bwd"] = (rc, so.dsee_last_error())
    rc = so.dsee_spade_resblock_train_fwd(n0, one, one, n1, one, one, None, one, lab, lab, shift, nc, one, one, 1e-5, 0.1, 0.2,
                                          N, R, R, Cc, one, big, one, big, None)
    out["dsee_spade_resblock_train_fwd"] = (rc, so.dsee_last_error())
    rc = so.dsee_spade_resblock_fwd(n0, one, one, n1, one, one, one, lab, lab, shift, nc, one, one, 0, 1, 1e-5, 0.1, 0.2, N, R, R, Cc,
                                    one, big, None)
    out["dsee_spade_resblock_fwd"] = (rc, so.dsee_last_error())
    return out


def _norm(fill):
    buf = ctypes.create_string_buffer(fill * 512, 512)     # a dsee_norm_layer: all-zero bytes = no table (SPADE), else SEAN
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_backward_refuses_a_label_map_that_does_not_cover_the_feature_map():
    """The backward pass sizes its one-hot buffer from H, W while dsee_label_onehot writes (lab_h >> shift) x (lab_w >> shift)
    pixels: a map of 128 x 128 >> 1 under a 128 x 128 feature map is refused by the backward entry like by the two forward
    entries, with and without a table."""
    from deepsee_amd import lib as L
    so = L.lib()
    for fill in (b"\x00", b"\x40"):
        keep, n = _norm(fill)
        for who, (rc, err) in _block_calls(so, n, n, 128, 1).items():
            assert rc != 0 and who.encode() + b":" in err and b"does not cover" in err, (who, rc, err)


def test_all_block_entry_points_refuse_a_spade_and_a_sean_norm_in_one_block():
    from deepsee_amd import lib as L
    so = L.lib()
    keep0, spade = _norm(b"\x00")
    keep1, sean = _norm(b"\x40")
    for n0, n1 in ((spade, sean), (sean, spade)):
        for who, (rc, err) in _block_calls(so, n0, n1, 128, 0).items():
            assert rc != 0 and who.encode() + b": both norm layers of a block are SPADE or both SEAN" in err, (who, rc, err)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps(_sizes(), indent=1))
