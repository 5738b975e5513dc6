"""dsee_generator_prepare / dsee_generator_fwd / dsee_style_table_fwd and deepsee_amd/native.py on the host.  Nothing here launches
a kernel: device pointers are the address 4096 and never dereferenced (every call below is refused by the argument check, which
reads the scalars and the host struct only)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from oracle import deepsee_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsee_style_table_fwd", "dsee_generator_prepared_bytes", "dsee_generator_fwd_workspace", "dsee_generator_prepare",
       "dsee_generator_fwd")
BASE = dict(start_size=32, crop_size=128, load_size=128, ngf=8, batchSize=4)
EINVAL, EUNSUPPORTED = -1, -3
ONE = C.c_void_p(4096)
BIG = 1 << 40


def desc_of(**over):
    from deepsee_amd import native
    from deepsee_amd.options import make_opt
    return native.layout(make_opt(**dict(BASE, **over)))[1]


def fwd(so, d, n=4, h=32, w=32, lab=None, out=ONE, prepared_bytes=BIG, workspace_bytes=BIG):
    lab = lab or (h << d.levels, w << d.levels)
    rc = so.dsee_generator_fwd(C.byref(d), ONE, ONE, prepared_bytes, ONE, ONE, lab[0], lab[1], ONE, out, n, h, w, ONE,
                               workspace_bytes, None)
    return rc, so.dsee_last_error()


def test_new_symbols_are_in_the_library_and_the_header():
    from deepsee_amd import lib as L
    protos = L.header_prototypes()
    so = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(so, name), name
    hdr = open(L.HEADER_PATH).read()
    assert "typedef struct dsee_generator_desc" in hdr and "DSEE_GEN_MAX_BLOCKS" in hdr


@pytest.mark.parametrize("over", [{}, {"norm_G": "spectralseansyncbatch3x3"}, {"label_nc": 5}, {"crop_size": 256, "load_size": 256}])
def test_layout_covers_what_the_generator_reads_and_pack_round_trips(over):
    from deepsee_amd import native
    from deepsee_amd.options import make_opt
    opt, oopt = make_opt(**dict(BASE, **over)), O.make_opt(**dict(BASE, **over))
    spec = O.net_specs(oopt)["SR"]
    # not read by the forward: BatchNorm's step counter, style_conv (defined by the reference, never used), the NoiseInjection
    # weights (training only)
    read = {k: tuple(s) for k, s in spec.items()
            if not (k.endswith("num_batches_tracked") or ".style_conv." in k or re.search(r"\.noise_(in|skip|middle)\.weight$", k))}
    entries, desc = native.layout(opt)
    assert {k: s for k, _, s in entries} == read and len(entries) == len(read)
    spans = sorted((o, o + max(1, native._numel(s))) for _, o, s in entries)
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= desc.param_floats
    assert all(o % native.ALIGN == 0 for o, _ in spans)
    state = O.recipe_state(oopt, gain=1.0)["SR"]
    flat = native.pack(state, opt, device="cpu")
    assert flat.numel() == desc.param_floats
    for k, o, s in entries:
        assert torch.equal(flat[o:o + native._numel(s)].reshape(s), state[k].float()), k
    # the descriptor names the same offsets
    off = {k: o for k, o, _ in entries}
    assert desc.initial_w == off["initial.weight"] and desc.conv_img_b == off["conv_img.bias"]
    assert desc.blocks[1].conv_1.weight_v == off["G_middle_0.conv_1.weight_v"]
    assert desc.blocks[1].norm_0.ws_beta == off["G_middle_0.norm_0.mlp_style_beta.weight"]
    assert desc.blocks[0].norm_1.running_var == off["head_0.norm_1.param_free_norm.running_var"]
    assert [desc.blocks[i].ups for i in range(desc.n_blocks)] == [0, 1, 0] + [1] * (desc.n_blocks - 3)


def test_size_functions_are_positive_and_monotone():
    from deepsee_amd import lib as L
    so = L.lib()
    assert so.dsee_generator_prepared_bytes(128, 19, 128, 4) > 0
    assert so.dsee_generator_prepared_bytes(512, 19, 128, 6) > so.dsee_generator_prepared_bytes(128, 19, 128, 6)
    prev = 0
    for n in (1, 2, 4, 8, 9):
        cur = so.dsee_generator_fwd_workspace(128, 19, 2, n, 32, 32)
        assert cur > 0 and cur >= prev, (n, cur, prev)
        prev = cur
    sizes = sorted(((h * w, so.dsee_generator_fwd_workspace(128, 19, 2, 4, h, w)) for h, w in
                    ((16, 16), (32, 32), (32, 64), (64, 32), (48, 48), (64, 64), (100, 60))))
    assert all(b > 0 for _, b in sizes)
    assert all(a[1] <= b[1] for a, b in zip(sizes, sizes[1:])), sizes


def test_refusals():
    from deepsee_amd import lib as L
    so = L.lib()
    d = desc_of()
    cases = {
        "LR 16 x 16": (fwd(so, d, n=16, h=16, w=16), EUNSUPPORTED, b"below 32 x 32"),
        "N = 1 at LR 32 x 32 (64 tiles)": (fwd(so, d, n=1), EUNSUPPORTED, b"N (H/4) (W/4) % 256 == 0"),
        "C = 64": (fwd(so, desc_of(ngf=4)), EUNSUPPORTED, b"C % 128 == 0"),
        "a SEAN level above max_fm_size": (fwd(so, desc_of(max_fm_size=64)), EUNSUPPORTED, b"max_fm_size = 64"),
        "label_nc = 33": (fwd(so, desc_of(label_nc=33)), EUNSUPPORTED, b"label_nc = 33"),
        "InstanceNorm norm_G": (fwd(so, desc_of(norm_G="spectralspadeinstance3x3")), EUNSUPPORTED, b"InstanceNorm"),
        "the 16-bit mode": (fwd(so, desc_of(precision="fp16")), EUNSUPPORTED, b"16-bit"),
        "the resnet generator": (fwd(so, desc_of(netG="nospadenostyle")), EUNSUPPORTED, b"ResnetBlock"),
        "the puresean generator": (fwd(so, desc_of(netG="puresean")), EUNSUPPORTED, b"PureSEAN"),
        "a label map that does not match h << levels": (fwd(so, d, lab=(64, 128)), EINVAL, b"label map (64 x 128)"),
        "a NULL pointer": (fwd(so, d, out=None), EINVAL, b"NULL argument"),
        "a workspace one byte too small": (fwd(so, d, workspace_bytes=so.dsee_generator_fwd_workspace(128, 19, 2, 4, 32, 32) - 1),
                                           EINVAL, b"(dsee_generator_fwd_workspace)"),
        "a prepared buffer one byte too small": (fwd(so, d, prepared_bytes=so.dsee_generator_prepared_bytes(128, 19, 128, 4) - 1),
                                                 EINVAL, b"(dsee_generator_prepared_bytes)"),
    }
    # a PureSEAN kind: the tail of load_size >= 512
    tail = desc_of(start_size=16, crop_size=512, load_size=512)
    assert [tail.blocks[i].kind for i in range(tail.n_blocks)][-1] == 2
    cases["a PureSEAN kind"] = (fwd(so, tail, n=16, h=16, w=16), EUNSUPPORTED, b"PureSEAN")
    for what, ((rc, err), want, fragment) in cases.items():
        assert rc == want and err.startswith(b"dsee_generator_fwd: ") and fragment in err, (what, rc, err)
    # order: a NULL pointer is reported before an unsupported shape, the shape before the label map, the label map before the sizes
    assert fwd(so, d, n=1, out=None)[0] == EINVAL
    assert fwd(so, d, n=1, lab=(64, 64), workspace_bytes=1)[0] == EUNSUPPORTED
    assert b"label map" in fwd(so, d, lab=(64, 64), workspace_bytes=1)[1]
    # prepare checks alike; the table kernel refuses shapes outside its rules before a launch
    rc = so.dsee_generator_prepare(C.byref(d), ONE, ONE, so.dsee_generator_prepared_bytes(128, 19, 128, 4) - 1, None)
    assert rc == EINVAL and b"dsee_generator_prepare: prepared buffer" in so.dsee_last_error()
    assert so.dsee_generator_prepare(C.byref(d), None, ONE, BIG, None) == EINVAL
    for n, l, s, rows in ((1, 0, 128, 64), (1, 33, 128, 64), (1, 19, 126, 64), (1, 19, 128, 96)):
        assert so.dsee_style_table_fwd(ONE, ONE, ONE, n, l, s, rows, None, None) == EUNSUPPORTED, (n, l, s, rows)
    assert so.dsee_style_table_fwd(ONE, None, ONE, 1, 19, 128, 64, None, None) == EINVAL


C_HOST = r"""
#include <stdio.h>
#include <string.h>
#include "deepsee_hip.h"

int main(void) {
  dsee_generator_desc d;
  memset(&d, 0, sizeof d);
  d.C = 128; d.label_nc = 19; d.S = 128; d.max_fm_size = 256; d.n_blocks = 4;
  d.norm = DSEE_GEN_NORM_BATCH; d.precision = DSEE_GEN_FP32;
  for (int i = 0; i < d.n_blocks; ++i) {
    d.blocks[i].kind = i ? DSEE_GEN_SEAN : DSEE_GEN_SPADE;
    d.blocks[i].ups = i == 1 || i == 3;
  }
  size_t pb = dsee_generator_prepared_bytes(d.C, d.label_nc, d.S, d.n_blocks);
  size_t wb = dsee_generator_fwd_workspace(d.C, d.label_nc, 2, 4, 32, 32);
  printf("prepared %zu workspace %zu desc %zu\n", pb, wb, sizeof d);
  int rc = dsee_generator_fwd(&d, NULL, NULL, pb, NULL, NULL, 128, 128, NULL, NULL, 4, 32, 32, NULL, wb, NULL);
  printf("rc %d: %s\n", rc, dsee_last_error());
  return rc == DSEE_EINVAL && pb > 0 && wb > 0 ? 0 : 1;
}
"""


def test_a_c_translation_unit_uses_the_header_and_the_library(tmp_path):
    """The header is valid C (compiled with -x c, not as C++), and a C host links against the built library."""
    from deepsee_amd import lib as L, native
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    src, exe = tmp_path / "host.c", tmp_path / "host"
    src.write_text(C_HOST)
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.run([hipcc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", libdir, "-ldeepsee_hip", "-Wl,-rpath," + libdir, "-o", str(exe)], check=True, capture_output=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "rc -1: dsee_generator_fwd: NULL argument" in run.stdout
    # the struct has the same size on both sides of the binding
    assert "desc %d\n" % C.sizeof(native.GeneratorDesc) in run.stdout
