"""The dense-block feature buffer (`own_dense_block`: strided 1x1 / 3x3 kernels on one channels_last buffer per block, no
torch.cat, input gradients accumulated inside the 1x1 gradient kernel) against the network it extends: a whole forward +
input gradient of DenseNet-121, bf16, channels_last, 512 structured images at 224 x 224, with `own_dense_pointwise` +
`own_dense_conv` (the code path as it was: the baseline, "off") and with `own_dense_block` next to them ("on"), in ONE
process on one tree, warmed up, in alternating rounds timed with device events.  The yardstick is the two-switch network of
the same run, never an earlier profile.  Writes profiles/dense_block_bench.json and a short profiles/dense_block_bench.md
and prints the JSON document.

usage: python tools/bench_dense_block.py [--batch 512] [--net-rounds 7] [--net-iters 2] [--out PATH.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_dense1x1 import random_bn_checkpoint  # noqa: E402
from bench_depthwise import events_us, forward_and_gradient, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    path = random_bn_checkpoint(os.path.join(tempfile.mkdtemp(prefix="adil_db_"), "densenet.pt"), dev)
    kw = dict(seed=0, weights=path, device=dev)
    models = {v: zoo.build_classifier("densenet121", dtype=torch.bfloat16, channels_last=True, own_dense_pointwise=True,
                                      own_dense_conv=True, own_dense_block=(v == "on"), **kw) for v in ("off", "on")}
    assert sum(isinstance(m, zoo._OwnDenseBlock) for m in models["on"].modules()) == 4
    out = {"what": "DenseNet-121 bf16 channels_last with own_dense_pointwise + own_dense_conv, %d structured images at 224 x 224, "
                   "forward + input gradient of sum(logits^2); own_dense_block off (the baseline of this run) / on, alternating "
                   "rounds of %d passes" % (b, args.net_iters)}
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
        for _ in range(2):
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
    d, w = out["ms_per_pass"]["off"], out["ms_per_pass"]["on"]
    out["switch_on_against_off"] = {"gain_ms_at_median": round(d["median"] - w["median"], 3),
                                    "gain_percent_at_median": round(100.0 * (d["median"] - w["median"]) / d["median"], 2),
                                    "larger_spread_ms": max(d["spread"], w["spread"]),
                                    "every_on_round_beats_every_off_round": bool(w["max"] < d["min"])}
    return out


def markdown(out):
    n = out["network"]
    d, w, s = n["ms_per_pass"]["off"], n["ms_per_pass"]["on"], n["switch_on_against_off"]
    a = n["against_the_fp32_network_on_16_images"]
    row = lambda name, t: "| %s | %.3f | %.3f | %.3f | %s |" % (name, t["median"], t["min"], t["max"], " ".join("%.1f" % u for u in t["rounds"]))
    return "\n".join([
        "# own_dense_block against the two-switch DenseNet-121", "",
        "Written by `tools/bench_dense_block.py` (the numbers are in `dense_block_bench.json` next to this file).", "",
        "- device: %s; kernel source hash %s" % (out["device"], out["kernel_source_hash"]),
        "- %s" % n["what"],
        "- timing: device events around %d passes per round, %d alternating rounds after 3 warm-up passes per variant, one "
        "process" % (out["iters_per_round"], out["rounds"]), "",
        "| variant | median ms / pass | min | max | rounds |", "|---|---|---|---|---|",
        row("own_dense_pointwise + own_dense_conv (baseline)", d), row("+ own_dense_block", w), "",
        "Gain at the median: %.3f ms (%.2f %%); larger spread of the two: %.3f ms; every round with the switch beats every round "
        "without it: %s." % (s["gain_ms_at_median"], s["gain_percent_at_median"], s["larger_spread_ms"],
                            s["every_on_round_beats_every_off_round"]), "",
        "Peak allocated memory of one pass: %.3f GiB without, %.3f GiB with the switch." % (
            n["peak_allocated_gib_of_one_pass"]["off"], n["peak_allocated_gib_of_one_pass"]["on"]), "",
        "Against the fp32 network on 16 images (rms logit %.4f, bf16 depth bound %.5f): mean |logit error| %.5f without / %.5f "
        "with; input-gradient relative error %.4f without / %.4f with." % (
            a["rms_logit"], a["bf16_depth_bound_121_layers"], a["off"]["mean_abs_logit_error"], a["on"]["mean_abs_logit_error"],
            a["off"]["input_gradient_relative_error"], a["on"]["input_gradient_relative_error"]), ""])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--net-rounds", type=int, default=7)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_block_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "own_dense_block on / off in DenseNet-121 with both dense switches, one process, alternating rounds, device "
                   "events; milliseconds per forward + input-gradient pass",
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.net_rounds,
           "iters_per_round": args.net_iters}
    out["network"] = bench_network(args, dev)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(markdown(out))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
