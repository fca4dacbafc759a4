#!/usr/bin/env python
"""Inference benchmark: the existing eval forward (the training decomposition with training=False) against
atomnas_amd.inference.InferenceModel (one fused launch per atomic block), eager and as a captured hipGraph, in ONE process on one GPU.

    python tools/infer_bench.py [--nets atomnas_c,atomnas_c_supernet,atomnas_mix_supernet] [--batches 1,8,64,256] [--blocks-at 256]
    python tools/infer_bench.py --nets atomnas_c_plus --batches 1,8,256 --blocks-at 1,8,256      # the SE blocks (profiles/infer_bench_se.txt)

bf16, 224 x 224, random weights and images (the time does not depend on the values).  Per (network, batch): warm-up, then `iters`
forwards between two device events, repeated `reps` times with the three variants ALTERNATING (other work shares the box); the median
over the repetitions is printed as ms per forward and images/s.  The compiled network fuses what the default policy fuses
(atomnas_block_infer_supported / atomnas_block_infer_se_supported; --policy all: everything the kernel can run).  Per block
(--blocks-at, one table per batch size): the block's own input, recorded from one forward, through the module's existing path and
through the fused kernel -- for EVERY block the kernel can run (atomnas_block_infer_runs; blocks with Squeeze-and-Excitation:
atomnas_block_infer_se_runs), the last column says whether the policy fuses it: this table is where the policy's rule comes from.
No GPU: the tool fails, it does not fall back.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = ("atomnas_c", "atomnas_c_supernet", "atomnas_mix_supernet")


def build_model(name):
    from atomnas_amd import configs
    from atomnas_amd.models import mobilenet_supernet as ms, searched_network as sn
    torch.manual_seed(1995)
    if name in ("atomnas_c", "atomnas_c_plus"):
        model = sn.Model(**dict(configs.searched_kwparams(name), input_size=224))
    else:
        model = ms.Model(**dict(configs.model_kwparams(name), input_size=224))
    with torch.no_grad():   # running statistics of a net that has seen data: keeps the activations in range through 22 blocks
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_var.fill_(1.0)
    return model.cuda().eval()


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def compare(variants, iters, reps, warmup):
    """variants: [(label, callable)] -> {label: median ms per call}, the variants alternating inside every repetition"""
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {label: [] for label, _ in variants}
    for _ in range(reps):
        for label, fn in variants:
            times[label].append(timed(fn, iters))
    return {label: statistics.median(v) for label, v in times.items()}


def iters_for(ms_estimate, target_ms=300.0):
    return max(5, min(500, int(target_ms / max(ms_estimate, 1e-3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default=",".join(NETS))
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--blocks-at", default="256", help="batch sizes of the per-block tables, comma separated (0: skip them)")
    ap.add_argument("--policy", default="measured", choices=("measured", "all"),
                    help="what the compiled network fuses: the blocks measured faster (default) or every block the kernel can run")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("infer_bench: no GPU (a timing needs the device; there is no CPU fallback)")
    from atomnas_amd import build
    from atomnas_amd import inference
    from atomnas_amd.inference import FusedBlock, compile_for_inference
    inference.POLICY = args.policy
    from atomnas_amd import _lib
    _lib.load()   # the library as built (python -m atomnas_amd.build); a missing one is an error, not a build on the timed box
    print("# infer_bench: %s, torch %s, lib %s" % (torch.cuda.get_device_name(0), torch.__version__, build.sources_digest()[:12]))
    print("# ms per forward = median of %d repetitions, variants alternating; images/s = batch / that; policy: %s" % (args.reps, args.policy))
    for name in args.nets.split(","):
        model = build_model(name)
        net = compile_for_inference(model)
        kinds = [k for _, k, _ in net.plan()]
        print("\n## %s: %d blocks fused, %d on the existing path" % (name, kinds.count("fused"), kinds.count("fallback")))
        print("%-22s %6s %14s %12s %12s %8s" % ("net", "batch", "variant", "ms/forward", "images/s", "vs eval"))
        for bs in [int(b) for b in args.batches.split(",") if b]:   # --batches "": the per-block tables only
            x = torch.randn(bs, 3, 224, 224, device="cuda")
            gnet = compile_for_inference(model, use_graph=True, batch_size=bs)
            with torch.no_grad():
                if float((net(x).float() - model(x).float()).abs().max()) > 0.5 * max(1.0, float(model(x).float().abs().max())):
                    sys.exit("infer_bench: the fused path disagrees with the eval forward on %s at batch %d" % (name, bs))

            def f_eval():
                with torch.no_grad():
                    model(x)
            variants = [("eval forward", f_eval), ("fused eager", lambda: net(x)), ("fused graph", lambda: gnet(x))]
            for _, fn in variants:
                fn()
            torch.cuda.synchronize()
            res = compare(variants, iters_for(timed(f_eval, 3)), args.reps, args.warmup)
            for label, _ in variants:
                print("%-22s %6d %14s %12.3f %12.0f %7.2fx" % (name, bs, label, res[label], bs * 1e3 / res[label], res["eval forward"] / res[label]))
            del gnet
        for bs in [int(b) for b in args.blocks_at.split(",") if int(b)]:
            print("\n### %s per block at batch %d (ms): existing path / fused kernel" % (name, bs))
            print("%-6s %-44s %10s %10s %8s %8s" % ("block", "shape", "existing", "fused", "ratio", "policy"))
            policy = dict((n, k) for n, k, _ in net.plan())
            from atomnas_amd import runtime
            mgr = runtime.manager_of(model)
            mgr.enter()   # as inside a whole forward: the weights are packed once per forward, not once per block call
            with torch.no_grad():
                y = model.features[0](torch.randn(bs, 3, 224, 224, device="cuda"))
                for bname, m, fb in net.block_steps():
                    xin = y
                    if fb is None and runtime.plan_of(m).nb:
                        fb = FusedBlock(bname, m)
                    y = m(xin)
                    shape = "%dx%d %d->%d s%d k%s hid %d%s" % (xin.shape[2], xin.shape[3], xin.shape[1], y.shape[1], m.stride, list(m.kernel_sizes),
                                                             sum(m.channels), " se %d" % fb.se_hid if fb is not None and fb.se else "")
                    if fb is None or not fb.supported(*[xin.shape[i] for i in (0, 2, 3)], profitable=False):
                        print("%-6s %-44s %10s %10s %8s" % (bname, shape, "-", "fallback", "-"))
                        continue
                    variants = [("existing", lambda: m(xin)), ("fused", lambda: fb(xin))]
                    res = compare(variants, iters_for(timed(variants[0][1], 3), 100.0), args.reps, args.warmup)
                    print("%-6s %-44s %10.4f %10.4f %7.2fx %8s" % (bname, shape, res["existing"], res["fused"], res["existing"] / res["fused"], policy[bname]))
            mgr.leave()
        del net, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
