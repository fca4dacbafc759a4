"""Step time of knowledge distillation (engine.TrainStep(teacher=)) on one box; not a test, not a gate.

    python tools/distillbench.py [warmup] [steps]

The searched AtomNAS-C network at batch 256 (bench.py's build and protocol: resident synthetic batch, captured graph, 20 warm-up and 100
timed steps) without a teacher, with AtomNAS-C+ as teacher and with the AtomNAS-C supernet as teacher, in two alternating runs of one
process; each teacher's eval forward alone at the same batch (captured, the same launches the step contains); and the
atomnas_ce_distill launch next to atomnas_ce_smooth at 256 x 1000.  The expectation to set the figures against: a distilling step costs
about the step without a teacher plus the teacher's eval forward.
"""
import gc
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STUDENT, BATCH = "atomnas_c", 256


def build_teacher(name, hp):
    from atomnas_amd import configs
    from atomnas_amd.models import mobilenet_base as mb
    from atomnas_amd.models import mobilenet_supernet as ms
    from atomnas_amd.models import searched_network as sn
    torch.manual_seed(7)
    if name in ("atomnas_c", "atomnas_c_plus"):
        t = sn.Model(**configs.searched_kwparams(name), input_size=hp["image_size"])
    else:
        t = ms.Model(**configs.model_kwparams(name), input_size=hp["image_size"])
    t.apply(mb.init_weights_mnas)
    t.set_compute_dtype(torch.bfloat16)
    return t.cuda().eval()


def batch_of(hp):
    g = torch.Generator(device="cuda").manual_seed(1995)
    x = torch.randn(BATCH, 3, hp["image_size"], hp["image_size"], device="cuda", generator=g)
    y = torch.randint(0, 1000, (BATCH,), device="cuda", generator=g)
    return x, y


def run_step(teacher_name, warmup, steps):
    import bench
    from atomnas_amd import engine
    model, ts, hp, opt, ema, pinfo = bench.build(STUDENT, torch.bfloat16, BATCH, seed=1995)
    teacher = None
    if teacher_name is not None:
        teacher = build_teacher(teacher_name, hp)
        ts = engine.TrainStep(model, opt, ema, pinfo, weight_decay=hp["weight_decay"], wd_method=hp["weight_decay_method"],
                              label_smoothing=hp["label_smoothing"], batch_size=BATCH, image_size=hp["image_size"], teacher=teacher,
                              distill_alpha=0.5, distill_temperature=2.0)
    ts.set_batch(*batch_of(hp))
    for _ in range(warmup):
        ts.step(lr=hp["base_lr"], rho=0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(lr=hp["base_lr"], rho=0.0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kd = " kd %.4f" % float(ts.kd) if ts.kd is not None else ""
    print("step    %-10s batch %3d  teacher %-20s %8.3f ms/step  %7.0f img/s  loss %.4f%s" % (
        STUDENT, BATCH, teacher_name or "-", 1e3 * dt / steps, BATCH * steps / dt, float(ts.loss[0]), kd), flush=True)
    del model, ts, opt, ema, pinfo, teacher
    gc.collect()
    torch.cuda.empty_cache()


def run_teacher_alone(name, warmup, steps):
    from atomnas_amd import configs, ops, runtime
    hp = configs.SEARCH_HPARAMS
    t = build_teacher(name, hp)
    runtime.manager_of(t).ensure()
    x, _ = batch_of(hp)
    out = torch.zeros(BATCH, ops.pad8(1000), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            t(x, logits_out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g), torch.no_grad():
        t(x, logits_out=out)
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        g.replay()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("forward %-20s batch %3d  eval, captured %24.3f ms  %7.0f img/s" % (name, BATCH, 1e3 * dt / steps, BATCH * steps / dt), flush=True)
    del t, g, out, x
    gc.collect()
    torch.cuda.empty_cache()


def run_launch(n=200):
    from atomnas_amd import ops
    B, K = 256, 1000
    g = torch.Generator(device="cuda").manual_seed(3)
    s = torch.randn(B, K, device="cuda", generator=g) * 3
    t = torch.randn(B, K, device="cuda", generator=g) * 3
    y = torch.randint(0, K, (B,), device="cuda", generator=g)
    loss, kd = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    dl = torch.empty(B, K, dtype=torch.bfloat16, device="cuda")
    topk = torch.zeros(2, dtype=torch.int32, device="cuda")
    for name, fn in (("atomnas_ce_smooth", lambda: ops.ce_smooth(s, y, 0.1, B, K, loss, dl, 1.0, topk)),
                     ("atomnas_ce_distill", lambda: ops.ce_distill(s, t, y, 0.1, 0.5, 2.0, B, K, loss, kd, dl, 1.0, topk))):
        for _ in range(20):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print("launch  %-20s %d x %d bf16 gradient  %8.2f us per launch (%d back to back)" % (name, B, K, 1e3 * e0.elapsed_time(e1) / n, n), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    warmup, steps = (int(argv[0]) if argv else 20), (int(argv[1]) if len(argv) > 1 else 100)
    teachers = (None, "atomnas_c_plus", "atomnas_c_supernet")
    for _ in range(2):
        for name in teachers:
            run_step(name, warmup, steps)
    for name in teachers[1:]:
        run_teacher_alone(name, warmup, steps)
    run_launch()
