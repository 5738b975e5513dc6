"""The C-ABI calls of one G + D step, as text: what a change of the Python side of the hot path (deepsee_amd/ops.py) must leave
alone.  `deepsee_amd.lib.call` is wrapped and every call becomes one line: the entry-point name, every scalar argument by value,
every tensor argument as dtype[shape] (or None), every byref(ConvGeom) as its key() -- no addresses.  `ops.scratch` is wrapped
too: the byte count of every workspace-size query it is fed with, and its tag, is a line of its own.

The scenario is the one() of tests/test_gpu_model.py::test_kernel_path_switches (batchSize=2, ngf=16, seed=3: one G step and one
D step from recipe_state, hip_graphs=False) under the default plan, under every entry of that file's SWITCHES, and with
precision="fp16" with half_norms on and off, and with netG="nospadenostyle" (the reflection border pass and InstNormRes, which the
default generator never runs) in both precisions.  The default-plan, the 16-bit and the nospadenostyle scenarios also get a SHA-256
over the generated image, every loss and every G and D parameter gradient.

    python tools/call_trace.py --out DIR [--scenarios default keep_v=False fp16 ...]    # one <scenario>.trace per scenario + index.json
    python tools/call_trace.py --compare DIR_A DIR_B [--again DIR_A2]                   # the table of profiles/ops_operand_refactor.md

Run it on two checkouts on the same machine and compare the directories.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.append(ROOT)       # (appended: a PYTHONPATH that names another checkout's package wins)

HASHED = ("default", "fp16", "fp16_two_term_norms", "nospadenostyle", "nospadenostyle_fp16")
DTYPES = {"torch.float32": "f32", "torch.float16": "f16", "torch.int16": "i16", "torch.int32": "i32", "torch.uint8": "u8",
          "torch.int64": "i64", "torch.bfloat16": "bf16", "torch.float64": "f64"}


def describe(a):
    import torch
    from deepsee_amd import lib as L
    if a is None:
        return "None"
    if isinstance(a, torch.Tensor):
        return "%s[%s]" % (DTYPES.get(str(a.dtype), str(a.dtype)), ",".join(str(s) for s in a.shape))
    if isinstance(a, C._SimpleCData):
        return repr(a.value)
    if isinstance(getattr(a, "_obj", None), L.ConvGeom):        # C.byref(geom)
        return "geom(%s)" % ",".join(str(v) for v in a._obj.key())
    if isinstance(a, bool):
        return repr(int(a))
    if isinstance(a, (int, float, str, bytes)):
        return repr(a)
    raise TypeError("call_trace: argument of type %s" % type(a).__name__)


class Recorder:
    """Wraps lib.call and ops.scratch while active; `lines` is the trace."""

    def __enter__(self):
        from deepsee_amd import lib as L, ops
        self.lines, self.L, self.ops = [], L, ops
        self.call, self.scratch = L.call, ops.scratch

        def call(name, *args):
            self.lines.append("%s(%s)" % (name, ", ".join(describe(a) for a in args)))
            return self.call(name, *args)

        def scratch(nbytes, tag="ws"):
            self.lines.append("scratch %s %d" % (tag, int(nbytes)))
            return self.scratch(nbytes, tag)

        L.call, ops.scratch = call, scratch
        return self

    def __exit__(self, *exc):
        self.L.call, self.ops.scratch = self.call, self.scratch


def scenarios():
    """[(name, make_opt overrides)]: default, every SWITCHES entry (tests/test_gpu_model.py), the two 16-bit modes, the resnet
    generator in both precisions."""
    from deepsee_amd import ops
    from tests.test_gpu_model import SWITCHES
    out = [("default", {})]
    for name, value in SWITCHES:
        if value is None:
            value = not getattr(ops.DEFAULT_PLAN, name)
        out.append(("%s=%s" % (name, value), dict(kernel_plan={name: value})))
    out.append(("fp16", dict(precision="fp16", kernel_plan=dict(half_norms=True))))
    out.append(("fp16_two_term_norms", dict(precision="fp16", kernel_plan=dict(half_norms=False))))
    out.append(("nospadenostyle", dict(netG="nospadenostyle")))
    out.append(("nospadenostyle_fp16", dict(netG="nospadenostyle", precision="fp16")))
    return out


def run(extra, hashed):
    """(trace lines, sha256 | None) of one G + D step."""
    import torch
    from oracle import deepsee_oracle as O
    from deepsee_amd.managers import TrainerManager
    from deepsee_amd.options import make_opt
    over = dict(batchSize=2, ngf=16, seed=3)
    if "netG" in extra:
        from tools.gen_golden_ablation import install_ablation
        install_ablation()          # (recipe_state in the state layout of the ablation generators; 'deepsee' keeps the oracle's own)
        over["netG"] = extra["netG"]
    batch = O.synthetic_batch(O.make_opt(**over), 2, seed=77)
    states = O.recipe_state(O.make_opt(**over), gain=1.0)
    tm = TrainerManager(make_opt(hip_graphs=False, **dict(over, **extra)))
    tm.sr_model.load_states(states)
    sha = hashlib.sha256()

    def feed(named):
        for k in sorted(named):
            sha.update(k.encode())
            v = named[k]
            sha.update(struct.pack("<d", v) if isinstance(v, float) else v.detach().cpu().contiguous().numpy().tobytes())

    def grads(opt):
        return {nm: (p.grad if p.grad is not None else torch.zeros_like(p)) for nm, p in zip(opt.names, opt.params)}

    with Recorder() as rec:
        tm.run_generator_one_step({k: v.clone() for k, v in batch.items()})
        torch.cuda.synchronize()
        feed({"fake": tm.get_latest_generated()})
        feed({k: float(v) for k, v in tm.g_losses.items()})
        feed(grads(tm.optimizer_G))
        tm.sr_model.load_states(states)
        rec.lines.append("-- D step")
        tm.run_discriminator_one_step({k: v.clone() for k, v in batch.items()})
        torch.cuda.synchronize()
        feed({k: float(v) for k, v in tm.d_losses.items()})
        feed(grads(tm.optimizer_D))
    tm.close()
    return rec.lines, (sha.hexdigest() if hashed else None)


def forms(lines):
    """Which Winograd-domain operand forms a trace reached, read from the entry points and the weight-gradient split codes.
    Arguments are counted by position in include/deepsee_hip.h's order (tensor shapes and geom keys hold no ", "):
    wino43_wgrad(V, dM, ws, nbytes, dw, t, cin, cout, co, ci, SPLIT, ...) -> 10; wino43_wgrad_table(V, dM, ws, nbytes, dw,
    dtable, t, nb, ca, rows, nc, SPLIT, ...) -> 11; gemm_f16x2_pre* / gemm_f16p_pre*(A, U, M, m, n, k, rows per group, weight
    rows, amax, BOUND, ...) -> 9.  An entry point that gains an argument in front of these needs the index moved."""
    seen = set()
    for ln in lines:
        name = ln.split("(", 1)[0]
        if name in ("wino43_wgrad", "wino43_wgrad_table"):
            code = int(ln[:-1].split(", ")[10 if name == "wino43_wgrad" else 11])
            seen.add({1: "bf16x3-T V", 5: "f16x2 V", 6: "f16x2 V", 7: "packed V"}.get(code, "fp32 V"))
            seen.add({1: "bf16x3-T dM", 6: "f16x2 dM", 7: "packed dM"}.get(code, "fp32 dM"))
        elif name.startswith(("gemm_f16x2_pre", "gemm_f16p_pre")) and "1.0" in ln.split(", ")[9:10]:
            seen.add("adjoint on %s dM" % ("packed" if "f16p" in name else "f16x2"))     # (scale bound DM_BOUND: A operand is a dM)
    return sorted(seen)


def compare(dir_a, dir_b, again):
    ia, ib = (json.load(open(os.path.join(d, "index.json"))) for d in (dir_a, dir_b))
    ia2 = json.load(open(os.path.join(again, "index.json"))) if again else None
    print("| scenario | calls, parent | calls, branch | traces | operand forms reached |")
    print("|---|---|---|---|---|")
    same = True
    for name in ia:
        a = open(os.path.join(dir_a, ia[name]["file"])).read().splitlines()
        b = open(os.path.join(dir_b, ib[name]["file"])).read().splitlines() if name in ib else []
        n = lambda t: sum(1 for ln in t if not ln.startswith(("scratch ", "-- ")))
        eq = a == b
        same &= eq
        if not eq:
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print("first difference of %s at line %d:\n  %s\n  %s" % (name, first + 1, a[first:first + 1], b[first:first + 1]),
                  file=sys.stderr)
        print("| %s | %d | %d | %s | %s |" % (name, n(a), n(b), "identical" if eq else "DIFFERENT", ", ".join(forms(a))))
    print()
    print("| scenario | SHA-256, parent | parent again | branch |")
    print("|---|---|---|---|")
    for name in ia:
        if ia[name].get("sha256"):
            h2 = ia2[name]["sha256"] if ia2 and name in ia2 else None
            hb = ib.get(name, {}).get("sha256")
            stable = h2 is None or h2 == ia[name]["sha256"]
            print("| %s | %s | %s | %s |" % (name, ia[name]["sha256"][:16], "same" if stable and h2 else (h2 or "-")[:16],
                                             "same" if hb == ia[name]["sha256"] else (hb or "-")[:16]))
            if stable and hb != ia[name]["sha256"]:
                same = False
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="directory for <scenario>.trace and index.json")
    ap.add_argument("--scenarios", nargs="*", help="names to run (default: all)")
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--again", help="a second run of DIR_A's checkout: which hashes are stable there")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.again))
    import torch
    assert torch.cuda.is_available() and a.out, "needs the MI355X and --out"
    torch.cuda.set_device(0)
    os.makedirs(a.out, exist_ok=True)
    index = {}
    for name, extra in scenarios():
        if a.scenarios and name not in a.scenarios:
            continue
        lines, sha = run(extra, name in HASHED)
        fn = name.replace("=", "-") + ".trace"
        with open(os.path.join(a.out, fn), "w") as f:
            f.write("\n".join(lines) + "\n")
        index[name] = {"file": fn, "calls": sum(1 for ln in lines if not ln.startswith(("scratch ", "-- "))), "sha256": sha}
        with open(os.path.join(a.out, "index.json"), "w") as f:
            json.dump(index, f, indent=1)
        print(json.dumps({name: index[name]}), flush=True)


if __name__ == "__main__":
    main()
