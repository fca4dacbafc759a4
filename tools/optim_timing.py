"""The two fused optimizer kernels on one arena of the AtomNAS-C supernet's size (11.2 M fp32 elements, EMA on, momentum 0.9, L2 value
on), alternating, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d out/optim -o k -- python tools/optim_timing.py [n] [reps]
    python tools/optim_timing.py --summary out/optim        # per-kernel mean / min / max / spread of the trace

Without the profiler the script prints event timings of the same launches (launch + kernel + the one-workgroup sum of the L2 value)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + d)
    per = {}
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"].split("(")[0]
                if "k_rmsprop_ema" in name or "k_sgd_ema" in name:
                    per.setdefault(name.split("::")[-1], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name, v in sorted(per.items()):
        v = v[len(v) // 5:]   # the first fifth is warm-up
        v.sort()
        mean = sum(v) / len(v)
        print("%-16s launches %4d  mean %8.2f us  median %8.2f  min %8.2f  max %8.2f  p10-p90 %.2f-%.2f" %
              (name, len(v), mean, v[len(v) // 2], v[0], v[-1], v[len(v) // 10], v[len(v) * 9 // 10]))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summary":
        return summary(sys.argv[2])
    import torch
    from atomnas_amd import ops
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 11200000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n = (n + 255) // 256 * 256
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    P, G, SQ, BUF, EMA = (torch.randn(n, device=dev, generator=g) * 0.05 for _ in range(5))
    SQ.abs_()
    wd = torch.full((n // 256,), 1e-5, device=dev)
    hyper = torch.tensor([1e-3, 0.0, 0.999, 1.0, 1.0, 0, 0, 0], dtype=torch.float32, device=dev)
    l2 = torch.zeros(1, device=dev)
    ws = torch.empty(4096, device=dev)

    def rms():
        ops.fused_rmsprop_ema(P, G, SQ, BUF, EMA, wd, n, hyper, 0.9, 1e-3, True, 0.9, l2_value=l2, ws=ws)

    def sgd():
        ops.fused_sgd_ema(P, G, BUF, EMA, wd, n, hyper, 0.9, True, l2_value=l2, ws=ws)
    t = {"rmsprop": [], "sgd": []}
    for i in range(reps):
        for name, fn in (("rmsprop", rms), ("sgd", sgd)):   # alternating: both see the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            t[name].append((e0, e1))
    torch.cuda.synchronize()
    for name, ev in t.items():
        v = sorted(a.elapsed_time(b) * 1e3 for a, b in ev[len(ev) // 5:])
        print("%-8s n %d  events: mean %.2f us  median %.2f  min %.2f  max %.2f" % (name, n, sum(v) / len(v), v[len(v) // 2], v[0], v[-1]))
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(l2).all())


if __name__ == "__main__":
    main()
