"""Throughput and peak memory of the accumulated training step (engine.TrainStep(accum_steps=A)) on bench.py's workload: the
AtomNAS-C supernet, bf16, one fixed synthetic batch per micro-batch, the learning rate and rho of bench.py's timed steps.

    python tools/bench_accum.py --accum 4 [--batch 256] [--steps 25] [--warmup 5]

prints ONE JSON line: images / s over all micro-batches, ms per optimizer step and per micro-batch, torch.cuda.max_memory_allocated.
Run it once per value of A (a process of its own: the peak is the process's) and next to `python bench.py` on the same box; bench.py
itself measures the plain step and is not touched by this tool."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--accum", type=int, default=4, help="micro-batches per optimizer step")
    ap.add_argument("--batch", type=int, default=256, help="micro-batch size")
    ap.add_argument("--steps", type=int, default=25, help="timed optimizer steps")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", default="atomnas_c_supernet")
    ap.add_argument("--no-graph", action="store_true")
    args = ap.parse_args()
    import bench
    from atomnas_amd import engine
    model, ts0, hp, opt, ema, pinfo = bench.build(args.model, torch.bfloat16, args.batch, seed=1995)
    del ts0   # bench.build's plain step: never ran, owns only its static batch
    ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=hp['weight_decay'], wd_method=hp['weight_decay_method'],
                          label_smoothing=hp['label_smoothing'], batch_size=args.batch, image_size=hp['image_size'],
                          use_graph=not args.no_graph, accum_steps=args.accum)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator(device="cuda").manual_seed(1995)
    x = torch.randn(args.batch, 3, hp['image_size'], hp['image_size'], device="cuda", generator=g)
    y = torch.randint(0, 1000, (args.batch,), device="cuda", generator=g)
    ts.set_batch(x, y)
    lr0, rho = hp['base_lr'], (1e-4 if pinfo is not None else 0.0)

    def one_step():
        for _ in range(args.accum - 1):
            ts.accumulate()
        ts.step(lr=lr0, rho=rho)

    first = None
    for i in range(max(args.warmup, 1)):
        one_step()
        if i == 0:
            first = float(ts.loss[0].item())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss, topk = ts.loss.tolist(), ts.topk.tolist()
    if not all(v == v and abs(v) < 1e6 for v in loss) or not all(0 <= t <= args.batch * args.accum for t in topk) or not loss[0] < first:
        raise SystemExit("bench_accum.py: the timed steps did not train (first CE %s, loss %s, top-k hits %s)" % (first, loss, topk))
    ms = dt / args.steps * 1e3
    print(json.dumps(dict(metric="images_per_s", value=round(args.batch * args.accum * args.steps / dt, 1), accum_steps=args.accum,
                          micro_batch=args.batch, ms_per_optimizer_step=round(ms, 3), ms_per_micro_batch=round(ms / args.accum, 3),
                          max_memory_allocated_mb=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), model=args.model,
                          use_graph=not args.no_graph, steps=args.steps, first_ce=round(first, 4), ce=round(loss[0], 4))))


if __name__ == "__main__":
    main()
