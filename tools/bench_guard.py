"""Cost of the guarded training step (engine.TrainStep(clip_norm=, skip_nonfinite=)) on bench.py's workload: the AtomNAS-C supernet,
bf16, one fixed synthetic batch, the learning rate and rho of bench.py's timed steps.

    python tools/bench_guard.py [--batch 256] [--steps 100] [--warmup 20] [--rounds 5]

Guard off and guard on run in ONE process on the same model and arenas, as TrainStep objects with graphs of their own, alternating
round by round (off, on, off2, off, on, off2, ...): each round times --steps / --rounds steps of one form between two device
synchronisations.  `off2` is a second un-guarded TrainStep, captured after the guarded one: two step graphs of the same launches differ
by where their buffers landed, and the difference between `off` and `off2` is that spread, which the guard's figure has to be read
against.  Prints ONE JSON line: per form the median and the minimum of the rounds' ms per step, the overhead of the guard against the
mean of the two un-guarded medians, the off / off2 spread, and the device time of the guard's own launches on the step's arenas (event
timed, back to back: the norm pass with its verdict, and the snapshot + restore + guarded EMA passes over the BatchNorm statistics).
The guarded form has both features on (skip_nonfinite, and a clip_norm so large that it never clips: the launches are the same whether
a step is clipped or not).  bench.py itself measures the plain step and is not touched by this tool."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100, help="timed steps per form, over all rounds (bench.py's default)")
    ap.add_argument("--warmup", type=int, default=20, help="warm-up steps per form (bench.py's default)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--model", default="atomnas_c_supernet")
    args = ap.parse_args()
    import bench
    from atomnas_amd import engine
    model, ts_off, hp, opt, ema, pinfo = bench.build(args.model, torch.bfloat16, args.batch, seed=1995)
    ts_on = engine.TrainStep(model, opt, ema, pinfo, weight_decay=hp['weight_decay'], wd_method=hp['weight_decay_method'],
                             label_smoothing=hp['label_smoothing'], batch_size=args.batch, image_size=hp['image_size'],
                             clip_norm=1e30, skip_nonfinite=True)
    ts_off2 = engine.TrainStep(model, opt, ema, pinfo, weight_decay=hp['weight_decay'], wd_method=hp['weight_decay_method'],
                               label_smoothing=hp['label_smoothing'], batch_size=args.batch, image_size=hp['image_size'])
    g = torch.Generator(device="cuda").manual_seed(1995)
    x = torch.randn(args.batch, 3, hp['image_size'], hp['image_size'], device="cuda", generator=g)
    y = torch.randint(0, 1000, (args.batch,), device="cuda", generator=g)
    forms = (("off", ts_off), ("on", ts_on), ("off2", ts_off2))
    lr0, rho = hp['base_lr'], (1e-4 if pinfo is not None else 0.0)
    for _, ts in forms:
        ts.set_batch(x, y)
    first = None
    for _, ts in forms:
        for i in range(max(args.warmup, 1)):
            ts.step(lr=lr0, rho=rho)
            if first is None:
                first = float(ts.loss[0].item())
    per_round = max(args.steps // args.rounds, 1)
    ms = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, ts in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per_round):
                ts.step(lr=lr0, rho=rho)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / per_round * 1e3)
    loss = ts_on.loss.tolist()
    st = ts_on.guard_state()
    if not all(v == v and abs(v) < 1e6 for v in loss) or not loss[0] < first or st["skipped"] != 0 or st["clipped"] != 0:
        raise SystemExit("bench_guard.py: the timed steps did not train (first CE %s, loss %s, guard %s)" % (first, loss, st))
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = 0.5 * (med["off"] + med["off2"])

    def device_us(fn, reps=200):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / reps * 1e3, 2)
    from atomnas_amd import ops
    mgr = ts_on.mgr
    scratch = torch.zeros(ops.GUARD_WORDS, dtype=torch.float32, device="cuda")   # not the step's vector: its counters stay as they are

    def stat_passes():
        ops.guard_restore(ts_on._sbase, mgr.S, mgr.nS, None, True)
        ops.guard_restore(mgr.S, ts_on._sbase, mgr.nS, scratch, False)
        ops.ema_update_guarded(mgr.SEMA, mgr.S, mgr.nS, mgr.hyper, scratch)
    norm_us = device_us(lambda: ops.grad_guard(mgr.G, mgr.nP, mgr.hyper, 1e30, True, scratch, ts_on._guard_ws))
    plain_ema_us = device_us(lambda: ops.ema_update(mgr.SEMA, mgr.S, mgr.nS, mgr.hyper))
    stats_us = device_us(stat_passes)
    print(json.dumps(dict(metric="guard_overhead_pct", value=round((med["on"] / base - 1.0) * 100, 3),
                          ms_per_step_off=dict(median=round(med["off"], 4), min=round(min(ms["off"]), 4)),
                          ms_per_step_on=dict(median=round(med["on"], 4), min=round(min(ms["on"]), 4)),
                          ms_per_step_off2=dict(median=round(med["off2"], 4), min=round(min(ms["off2"]), 4)),
                          overhead_us=round((med["on"] - base) * 1e3, 1), off_off2_spread_us=round((med["off2"] - med["off"]) * 1e3, 1),
                          norm_pass_us=norm_us, norm_pass_tb_per_s=round(4.0 * mgr.nP / (norm_us * 1e-6) / 1e12, 2),
                          stat_passes_us=stats_us, plain_stat_ema_us=plain_ema_us, stat_floats=int(mgr.nS),
                          rounds=args.rounds, steps_per_round=per_round,
                          warmup=args.warmup, batch=args.batch, model=args.model, gradient_floats=int(ts_on.mgr.nP),
                          gnorm=round(st["norm"], 4), first_ce=round(first, 4), ce=round(loss[0], 4))))


if __name__ == "__main__":
    main()
