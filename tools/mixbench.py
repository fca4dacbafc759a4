"""Measurements of the depthwise 9 x 9 / 11 x 11 family (csrc/dwconv_big.hip); not a test, not a gate.

    python tools/mixbench.py shapes [N]          per-shape times of k = 7 / 9 / 11 through the C ABI (bf16, slab-major, stride 1, the hidden
                                                 widths of the mix supernet at 56^2 / 28^2 / 14^2 / 7^2), next to torch's own depthwise
                                                 convolution on the GPU and to the k = 7 time scaled by 81/49 and 121/49
    python tools/mixbench.py step [batch] [steps] training step of configs.model_kwparams('atomnas_mix_supernet') (bench.py's own build and
                                                 protocol: resident synthetic batch, captured graph; bench.py's --model list is closed, so the
                                                 mix supernet is timed from here), one JSON line
"""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def shapes(N):
    from atomnas_amd import ops
    from atomnas_amd.ops import Slab
    NSET, ITERS = 3, 10   # rotate over tensor sets: the Infinity Cache must not serve re-runs
    print("batch %d, bf16, stride 1, slab-major operands; ms per call (mean of %d, %d tensor sets)" % (N, ITERS, NSET))
    print("%-14s %9s %9s %9s %9s | %9s %9s" % ("shape", "fwd", "bwd", "k7-scaled", "k7-scaled", "torch fwd", "torch bwd"))
    for H, C in ((56, 144), (28, 240), (14, 480), (7, 1152)):
        base = {}
        for k in (7, 9, 11):
            M = N * H * H
            mk = lambda: Slab.from_plain(torch.randn(M, C, device="cuda").bfloat16())
            sets = [(mk(), mk(), mk(), mk()) for _ in range(NSET)]
            w = torch.randn(k * k, C, device="cuda")
            sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
            c1, c2, c3 = torch.rand(C, device="cuda"), torch.randn(C, device="cuda") * 0.1, torch.randn(C, device="cuda") * 0.1
            rows = ops.stat_rows_for(C)
            st, dw = torch.empty(rows * 2 * C, device="cuda"), torch.zeros(C * k * k, device="cuda")
            ws = torch.empty(rows * C * k * k, device="cuda")
            cnt = [0]

            def fwd():
                x, y, g, h = sets[cnt[0] % NSET]
                cnt[0] += 1
                ops.dwconv_fwd(x, sc, sh, True, w, y, st, C, N, H, H, C, k, 1, stat_rows=rows)

            def bwd():
                x, y, g, h = sets[cnt[0] % NSET]
                cnt[0] += 1
                ops.dwconv_bwd(g, y, c1, c2, c3, x, sc, sh, True, w, h, dw, st, C, N, H, H, C, k, 1, stat_rows=rows, dw_ws=ws)
            tf, tb = timed(fwd, ITERS), timed(bwd, ITERS)
            del sets
            # torch: the same convolution alone (no fused BatchNorm / activation / statistics), channels-last bf16
            xt = torch.randn(N, C, H, H, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            wt = torch.randn(C, 1, k, k, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
            yt = F.conv2d(xt, wt, None, 1, (k - 1) // 2, 1, C)
            gt = torch.randn_like(yt)
            ttf = timed(lambda: F.conv2d(xt, wt, None, 1, (k - 1) // 2, 1, C), 5)
            ttb = timed(lambda: torch.autograd.grad(yt, (xt, wt), gt, retain_graph=True), 5)
            del xt, wt, yt, gt
            if k == 7:
                base = dict(f=tf, b=tb)
            sf = base["f"] * k * k / 49.0
            sb = base["b"] * k * k / 49.0
            print("H%-3d C%-4d k%-2d %9.3f %9.3f %9.3f %9.3f | %9.3f %9.3f" % (H, C, k, tf, tb, sf, sb, ttf, ttb), flush=True)


def step(batch, steps):
    import bench
    model, ts, hp, opt, ema, pinfo = bench.build("atomnas_mix_supernet", torch.bfloat16, batch, seed=1995)
    g = torch.Generator(device="cuda").manual_seed(1995)
    x = torch.randn(batch, 3, hp["image_size"], hp["image_size"], device="cuda", generator=g)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    ts.set_batch(x, y)
    for _ in range(5):
        ts.step(lr=hp["base_lr"], rho=1e-4)
    torch.cuda.synchronize()
    first = ts.loss.tolist()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(lr=hp["base_lr"], rho=1e-4)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(model="atomnas_mix_supernet", batch=batch, steps=steps, ms_per_step=round(1e3 * dt / steps, 3),
                          images_per_sec=round(batch * steps / dt, 1), n_macs=int(model.n_macs), loss_first=first, loss_last=ts.loss.tolist(),
                          peak_mem_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "shapes"
    if mode == "shapes":
        shapes(int(sys.argv[2]) if len(sys.argv) > 2 else 256)
    else:
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
