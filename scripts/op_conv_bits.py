#!/usr/bin/env python3
"""SHA-256 of what mimo_op_conv3x3_forward / _dgrad return (z, BatchNorm statistics, dx) on the seeded inputs of
tests/test_ops_gpu.py, to compare two builds of libmimo_hip.so bit for bit.

    MIMO_HIP_LIB=<other build>/libmimo_hip.so python scripts/op_conv_bits.py dump other.txt
    python scripts/op_conv_bits.py dump this.txt
    python scripts/op_conv_bits.py compare other.txt this.txt      (exit status 1 when a line differs)

The cases write every layout of the weight packer (PackKind, mimo_unet_amd/csrc/pack_layout.h): the fp32 image, fp16 / bf16
pairs with and without the tap-paired last chunk and, with the wide decomposition forced on small layers as
tests/test_variants_gpu.py::conv_wide_forced does (MIMO_CONV_WIDE=2, in a child process: the switch is read once), the
pair and single-value wide layouts with more packed rows than mapped ones and a short channel tail.
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRED = [(3, 6, 7, 16, 33), (1, 2, 2, 8, 16), (2, 24, 24, 13, 75), (1, 40, 40, 75, 30)]
GROUPS = {
    # group: (MIMO_CONV_WIDE, precisions, cases (N, H, W, Cin, Cout))
    "default": (None, {"fp32": [(1, 3, 5, 4, 4), (3, 6, 7, 16, 33)], "split16": PAIRED, "bf16": PAIRED}),
    "wide": ("2", {p: [(1, 64, 96, 45, 30), (1, 37, 53, 40, 100)] for p in ("split16", "bf16-mixed", "16-mixed")}),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_group(name):
    import torch

    from mimo_unet_amd import _lib as L

    wide, by_precision = GROUPS[name]
    assert os.environ.get("MIMO_CONV_WIDE") == wide, "group %s runs with MIMO_CONV_WIDE=%s" % (name, wide)
    lib, st = L.load(), L.current_stream()
    for precision, cases in by_precision.items():
        prec = L.PRECISIONS[precision]
        for case in cases:
            N, H, W, Ci, Co = case
            g = torch.Generator().manual_seed(sum(case))  # test_conv3x3_forward_dgrad_wgrad's inputs
            x = torch.randn(N, Ci, H, W, generator=g)
            w = (torch.randn(Co, Ci, 3, 3, generator=g) / (3.0 * Ci ** 0.5)).cuda().contiguous()
            b = torch.randn(Co, generator=g).cuda()
            dz = torch.randn(N, Co, H, W, generator=g)
            # (channel padding as the plan stores it: 4-channel pixels for an image of <= 4 channels, 8-channel units otherwise)
            cip, cop = (Ci + 3) // 4 * 4 if Ci <= 4 else (Ci + 7) // 8 * 8, (Co + 7) // 8 * 8
            xd = torch.zeros(N, H, W, cip)
            xd[..., :Ci] = x.permute(0, 2, 3, 1)
            dzd = torch.zeros(N, H, W, cop)
            dzd[..., :Co] = dz.permute(0, 2, 3, 1)
            xd, dzd = xd.cuda(), dzd.cuda()
            nan = float("nan")
            z = torch.full((N, H, W, cop), nan, device="cuda")
            stats = torch.full((2, Co), nan, dtype=torch.float64, device="cuda")
            dx = torch.full((N, H, W, cip), nan, device="cuda")
            L.check(lib.mimo_op_conv3x3_forward(xd.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), stats.data_ptr(), N, H, W, Ci,
                                                cip, Co, cop, prec, st), "conv fwd")
            L.check(lib.mimo_op_conv3x3_dgrad(dzd.data_ptr(), w.data_ptr(), dx.data_ptr(), N, H, W, Ci, cip, Co, cop, prec, st), "conv dgrad")
            torch.cuda.synchronize()
            tag = "%s %s %s" % (name, precision, "x".join(map(str, case)))
            for what, t in (("z", z), ("stats", stats), ("dx", dx)):
                assert not torch.isnan(t).any(), (tag, what)
                print("%s %s %s" % (tag, what, sha(t)), flush=True)


def dump(path):
    lines = []
    for name, (wide, _) in GROUPS.items():
        env = {k: v for k, v in os.environ.items() if k != "MIMO_CONV_WIDE"}
        if wide is not None:
            env["MIMO_CONV_WIDE"] = wide
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "group", name], env=env, cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("group %s failed (exit status %d):\n%s%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:]))
        lines += r.stdout.splitlines()
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("%d hashes -> %s" % (len(lines), path))


def compare(path_a, path_b):
    a, b = ({l.rsplit(" ", 1)[0]: l.rsplit(" ", 1)[1] for l in open(p).read().splitlines()} for p in (path_a, path_b))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in bad:
        print("DIFFERENT %s: %s / %s" % (k, a.get(k, "missing"), b.get(k, "missing")))
    print("%d of %d outputs identical" % (len(set(a) | set(b)) - len(bad), len(set(a) | set(b))))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "group":
        run_group(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
