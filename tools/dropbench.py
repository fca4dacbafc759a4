"""Step time with and without stochastic depth (drop_connect_rate) on one box; not a test, not a gate.

    python tools/dropbench.py [warmup] [steps] [rate]

The AtomNAS-C supernet at batch 256 and AtomNAS-C+ (searched network, fused SE / Swish blocks) at batch 128, each with rate 0 and
rate 0.2 in two alternating runs (0, r, 0, r) of one process, with bench.py's own build and protocol (resident synthetic batch, captured
graph, 20 warm-up and 100 timed steps).  Prints one line per run with ms/step and the number of blocks that drop.
"""
import gc
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(name, batch, rate, warmup, steps):
    import bench
    model, ts, hp, opt, ema, pinfo = bench.build(name, torch.bfloat16, batch, seed=1995)
    model.set_drop_connect_rate(rate)
    dropping = sum(1 for b in model.get_named_block_list().values() if b.use_res_connect and b.drop_connect_rate > 0)
    g = torch.Generator(device="cuda").manual_seed(1995)
    x = torch.randn(batch, 3, hp["image_size"], hp["image_size"], device="cuda", generator=g)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=g)
    ts.set_batch(x, y)
    for _ in range(warmup):
        ts.step(lr=hp["base_lr"], rho=1e-4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(lr=hp["base_lr"], rho=1e-4)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = ts.loss.tolist()
    print("%-20s batch %3d  drop_connect_rate %.2f  dropping blocks %2d  %8.3f ms/step  loss %.4f" % (
        name, batch, rate, dropping, 1e3 * dt / steps, loss[0]), flush=True)
    del model, ts, opt, ema, pinfo, x, y
    gc.collect()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    argv = sys.argv[1:]
    warmup, steps = (int(argv[0]) if argv else 20), (int(argv[1]) if len(argv) > 1 else 100)
    rate = float(argv[2]) if len(argv) > 2 else 0.2
    for name, batch in (("atomnas_c_supernet", 256), ("atomnas_c_plus", 128)):
        for r in (0.0, rate, 0.0, rate):
            run(name, batch, r, warmup, steps)
