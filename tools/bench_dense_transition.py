"""The pool-first transition kernels (`ops.dense_transition`, `own_dense_transition`) and the stem wiring
(`own_dense_stem`) against the code they replace, in ONE process on one tree with seeded inputs, timed with device events.

Per layer: the three transition shapes of DenseNet-121 at 224 x 224, `ops.dense1x1_conv` (identity behind the convolution)
+ `F.avg_pool2d` and their autograd input gradient (the sequence as it was) against `ops.dense_transition`, alternating,
medians in microseconds, each also as a fraction of the 5.1 TB/s copy yardstick on the algorithmic bytes of the pool-first
form (forward x + y/4, gradient g/4 + xin + gx).

Whole network: forward + input gradient of sum(logits^2) on structured images, the three earlier dense switches (unchanged
code: the baseline of this run) against + transition, + stem and + both, in alternating rounds; peak allocated memory of
one pass; logit and input-gradient error against the fp32 network on 16 images.  The yardstick is always the baseline of
the same run, never an earlier profile.  Writes profiles/dense_transition_bench.json and .md and prints the JSON document.

usage: python tools/bench_dense_transition.py [--batch 512] [--net-rounds 7] [--net-iters 2] [--out PATH.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_dense1x1 import random_bn_checkpoint  # noqa: E402
from bench_depthwise import events_us, forward_and_gradient, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

COPY_TB_S = 5.1                                   # the copy yardstick of DESIGN.md section 4
SHAPES = [(56, 256, 128), (28, 512, 256), (14, 1024, 512)]       # (H = W of the input, K, N) at 224 x 224
VARIANTS = {"baseline": {}, "+transition": {"own_dense_transition": True}, "+stem": {"own_dense_stem": True},
            "+both": {"own_dense_transition": True, "own_dense_stem": True}}


def _stats(ts, nbytes):
    s = sorted(ts)
    med = s[len(s) // 2]
    return {"median_us": round(med, 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2),
            "fraction_of_copy_yardstick": round(nbytes / (med * 1e-6) / (COPY_TB_S * 1e12), 3), "rounds_us": [round(t, 2) for t in ts]}


def bench_layers(args, dev):
    res = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    b = args.batch
    for hw, k, n in SHAPES:
        rn = lambda *s: torch.randn(*s, generator=gen, device=dev)
        x = rn(b, hw, hw, k).bfloat16().permute(0, 3, 1, 2).requires_grad_(True)       # channels_last storage
        g = rn(b, hw // 2, hw // 2, n).bfloat16().permute(0, 3, 1, 2)
        w2d = (rn(n, k) * k ** -0.5).bfloat16().contiguous()
        wt2d = w2d.t().contiguous()
        sign = (torch.randint(0, 2, (k,), generator=gen, device=dev) * 2 - 1).float()
        ps = (0.7 + 0.6 * torch.rand(k, generator=gen, device=dev)) * sign
        pb = 0.2 * rn(k)
        one, zero = torch.ones(n, device=dev), torch.zeros(n, device=dev)
        fwd = {"old": lambda: F.avg_pool2d(ops.dense1x1_conv(x, ps, pb, w2d, wt2d, one, zero, False), 2),
               "new": lambda: ops.dense_transition(x, ps, pb, w2d, wt2d)}
        ys = {v: f() for v, f in fwd.items()}
        bwd = {v: (lambda y=y: torch.autograd.grad(y, x, g, retain_graph=True)) for v, y in ys.items()}
        yo, yn = ys["old"].detach().float(), ys["new"].detach().float()
        err = float((yn - yo).abs().max() / yo.abs().max())
        nb_f = 2 * (b * hw * hw * k + b * (hw // 2) ** 2 * n)
        nb_b = 2 * (b * (hw // 2) ** 2 * n + 2 * b * hw * hw * k)
        row = {"shape": "%d -> %d at %d x %d" % (k, n, hw, hw), "batch": b, "algorithmic_bytes": {"forward": nb_f, "gradient": nb_b},
               "max_abs_difference_new_old_relative_to_max_abs": round(err, 5)}
        for name, fns, nbytes in (("forward", fwd, nb_f), ("gradient", bwd, nb_b)):
            with torch.set_grad_enabled(name == "gradient"):
                for f in fns.values():
                    for _ in range(3):
                        f()
                ts = {v: [] for v in fns}
                for _ in range(args.rounds):
                    for v, f in fns.items():
                        ts[v].append(events_us(f, args.iters))
            row[name] = {v: _stats(t, nbytes) for v, t in ts.items()}
            row[name]["new_over_old_at_median"] = round(row[name]["new"]["median_us"] / row[name]["old"]["median_us"], 3)
        res.append(row)
        del x, g, ys, bwd, fwd
        torch.cuda.empty_cache()
    return res


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_dt_"), "densenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    three = dict(dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True)
    models = {v: zoo.build_classifier("densenet121", **three, **extra, **kw) for v, extra in VARIANTS.items()}
    assert sum(m.pool_first for m in models["+both"].modules() if isinstance(m, zoo._OwnTransition)) == 3
    assert isinstance(models["+both"][0].features, zoo._OwnDenseStem)
    out = {"what": "DenseNet-121 bf16 channels_last with own_dense_pointwise + own_dense_conv + own_dense_block (the baseline of "
                   "this run), %d structured images at 224 x 224, forward + input gradient of sum(logits^2); + own_dense_transition, "
                   "+ own_dense_stem, + both, alternating rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("densenet121", **kw)
    xs = images[:16].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_16_images"] = {"rms_logit": rms, "bf16_depth_bound_121_layers": 2.0 * 2.0 ** -9 * 121 ** 0.5 * rms,
                                                    **acc}
    del ref, lr, gr
    x = images.to(dev).bfloat16()

    def one(v):
        xi = x.detach().requires_grad_(True)
        logits = models[v](xi).float()
        torch.autograd.grad(logits.square().sum(), xi)

    peak = {}
    for v in models:
        for _ in range(3):
            one(v)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        one(v)
        torch.cuda.synchronize()
        peak[v] = round(torch.cuda.max_memory_allocated(dev) / 2.0 ** 30, 3)
    out["peak_allocated_gib_of_one_pass"] = peak
    times = {v: [] for v in models}
    for _ in range(args.net_rounds):
        for v in models:
            times[v].append(events_us(lambda: one(v), args.net_iters) / 1e3)
    out["ms_per_pass"] = {v: {"median": round(sorted(t)[len(t) // 2], 3), "min": round(min(t), 3), "max": round(max(t), 3),
                              "spread": round(max(t) - min(t), 3), "rounds": [round(u, 3) for u in t]} for v, t in times.items()}
    d = out["ms_per_pass"]["baseline"]
    out["against_the_baseline"] = {
        v: {"gain_ms_at_median": round(d["median"] - w["median"], 3),
            "gain_percent_at_median": round(100.0 * (d["median"] - w["median"]) / d["median"], 2),
            "larger_spread_ms": max(d["spread"], w["spread"]),
            "every_round_with_beats_every_round_without": bool(w["max"] < d["min"])}
        for v, w in out["ms_per_pass"].items() if v != "baseline"}
    return out


def markdown(out):
    n = out["network"]
    a = n["against_the_fp32_network_on_16_images"]
    lines = ["# Pool-first transitions and the fused stem against the three-switch DenseNet-121", "",
             "Written by `tools/bench_dense_transition.py` (the numbers are in `dense_transition_bench.json` next to this file).", "",
             "- device: %s; kernel source hash %s" % (out["device"], out["kernel_source_hash"]),
             "- per layer: batch %d, medians of %d alternating rounds of %d calls after 3 warm-up calls, device events; `old` = "
             "`ops.dense1x1_conv` + `F.avg_pool2d` (and their autograd gradient), `new` = `ops.dense_transition`; the fraction is of "
             "the %.1f TB/s copy yardstick on the pool-first algorithmic bytes" % (out["layers"][0]["batch"], out["layer_rounds"],
                                                                                 out["layer_iters"], COPY_TB_S), "",
             "| shape | direction | old us | new us | new / old | old fraction | new fraction |", "|---|---|---|---|---|---|---|"]
    for r in out["layers"]:
        for d in ("forward", "gradient"):
            t = r[d]
            lines.append("| %s | %s | %.1f | %.1f | %.3f | %.3f | %.3f |" % (
                r["shape"], d, t["old"]["median_us"], t["new"]["median_us"], t["new_over_old_at_median"],
                t["old"]["fraction_of_copy_yardstick"], t["new"]["fraction_of_copy_yardstick"]))
    lines += ["", "- %s" % n["what"],
              "- timing: device events around %d passes per round, %d alternating rounds after 3 warm-up passes per variant, one "
              "process" % (out["net_iters_per_round"], out["net_rounds"]), "",
              "| variant | median ms / pass | min | max | gain ms | gain % | every round beats every baseline round | peak GiB | "
              "logit error | gradient error |", "|---|---|---|---|---|---|---|---|---|---|"]
    for v, t in n["ms_per_pass"].items():
        s = n["against_the_baseline"].get(v)
        lines.append("| %s | %.3f | %.3f | %.3f | %s | %s | %s | %.3f | %.5f | %.4f |" % (
            v, t["median"], t["min"], t["max"], "%.3f" % s["gain_ms_at_median"] if s else "",
            "%.2f" % s["gain_percent_at_median"] if s else "", s["every_round_with_beats_every_round_without"] if s else "",
            n["peak_allocated_gib_of_one_pass"][v], a[v]["mean_abs_logit_error"], a[v]["input_gradient_relative_error"]))
    lines += ["", "Errors are against the fp32 network on 16 images (rms logit %.4f, bf16 depth bound %.5f): mean |logit error| and "
              "input-gradient relative error." % (a["rms_logit"], a["bf16_depth_bound_121_layers"]), ""]
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--net-rounds", type=int, default=7)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_transition_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {"what": "pool-first transition kernels and the DenseNet stem wiring against the code they replace, one process, "
                   "alternating rounds, device events",
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "layer_rounds": args.rounds,
           "layer_iters": args.iters, "net_rounds": args.net_rounds, "net_iters_per_round": args.net_iters}
    out["layers"] = bench_layers(args, dev)
    out["network"] = bench_network(args, dev)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(markdown(out))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
