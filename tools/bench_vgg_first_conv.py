"""VGG11's first group (Normalize, conv 3 -> 64, ReLU, 2x2 max-pool) on the fused kernels (`own_vgg_first_conv`:
adil_first3x3_pool_fwd / _bwd) against the parent's route (`own_vgg_conv` alone: Normalize in torch, the library
convolution, adil_bias_relu_pool2_fwd / _bwd), timed in ONE process, alternating, every shape warmed up, with device
events, on --batch images at 224 x 224 in bf16:
  (a) group 1 alone: forward (with the autograd graph recorded, as the attack runs it) and input gradient down to the
      attack's own NCHW tensor, median [min .. max] of the rounds, and each fused kernel's share of its byte bound
      (algorithmic bytes from the shapes over the flat-copy rate of profiles/r04_stream_patterns.md; reported, not asserted);
  (b) the whole bf16 VGG11 forward + input gradient of sum(logits^2), new switch off (the yardstick) against on, with the
      peak allocated memory of a pass.
"Faster" is claimed only where EVERY round of the new route is below EVERY round of the other.  Needs a GPU.
Writes profiles/vgg_first_conv_bench.json and .md (or --out) and prints the JSON.

usage: python tools/bench_vgg_first_conv.py [--batch 256] [--rounds 5] [--iters 5] [--net-rounds 5] [--net-iters 2] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_depthwise import events_us, forward_and_gradient, structured_batch  # noqa: E402
from bench_vgg_conv import summary  # noqa: E402
from dl_attack_on_imagenet_amd import zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

BF16 = torch.bfloat16
FLAT_COPY_TB_S = 5.1             # profiles/r04_stream_patterns.md
SIZE = 224


def byte_bounds(b, hw=SIZE):
    """Algorithmic bytes of the fused pair on bf16 streams: the image, the pooled 64-channel tensor, one index byte per
    pooled element; the same three tensors in both directions."""
    image, pooled = b * 3 * hw * hw * 2, b * (hw // 2) ** 2 * 64 * 2
    total = image + pooled + pooled // 2
    return {"image": image, "pooled": pooled, "idx": pooled // 2, "total": total,
            "us_at_flat_copy_rate": round(total / (FLAT_COPY_TB_S * 1e12) * 1e6, 1)}


def verdict(new, old):
    return "faster" if new["max"] < old["min"] else "slower" if new["min"] > old["max"] else "not separated"


def build(dev):
    kw = dict(seed=0, device=dev, dtype=BF16, channels_last=True, own_vgg_conv=True)
    return {"off": zoo.build_classifier("vgg11", **kw), "on": zoo.build_classifier("vgg11", own_vgg_first_conv=True, **kw)}


def bench_group(args, dev, models):
    b = args.batch
    x = structured_batch(b).to(dev).bfloat16().requires_grad_(True)
    g = torch.randn(b, SIZE // 2, SIZE // 2, 64, generator=torch.Generator().manual_seed(1)).bfloat16().to(dev).permute(0, 3, 1, 2)
    norm, feats_off, feats_on = models["off"][0], models["off"][1].features, models["on"][0].features
    fwd = {"parent": lambda: feats_off.first_group(norm(x)), "fused": lambda: feats_on.first_group(x)}
    keep = {k: f() for k, f in fwd.items()}
    fns = {"fused_fwd": fwd["fused"], "parent_fwd": fwd["parent"],
           "fused_bwd": lambda: torch.autograd.grad(keep["fused"], x, g, retain_graph=True),
           "parent_bwd": lambda: torch.autograd.grad(keep["parent"], x, g, retain_graph=True)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    diff = {"fwd": float((keep["fused"].float() - keep["parent"].float()).abs().max()),
            "bwd": float((fns["fused_bwd"]()[0].float() - fns["parent_bwd"]()[0].float()).abs().max())}
    times = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            times[k].append(events_us(fn, args.iters))
    us = {k: summary(t) for k, t in times.items()}
    bound = byte_bounds(b)
    return {"B": b, "H": SIZE, "W": SIZE, "us": us, "byte_bound": bound,
            "share_of_byte_bound_at_median": {d: round(bound["us_at_flat_copy_rate"] / us["fused_" + d]["median"], 3)
                                              for d in ("fwd", "bwd")},
            "max_abs_diff_fused_vs_parent": diff,
            "fused_against_parent": {d: verdict(us["fused_" + d], us["parent_" + d]) for d in ("fwd", "bwd")}}


def bench_network(args, dev, models):
    b = args.batch
    images = structured_batch(b)
    ref = zoo.build_classifier("vgg11", seed=0, device=dev)
    xs = images[:8].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    acc = {}
    for v, model in models.items():
        lg, gv = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((lg - lr).abs().mean()),
                  "input_gradient_relative_error": float((gv - gr).norm() / gr.norm())}
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
        torch.cuda.reset_peak_memory_stats()
        one(v)
        torch.cuda.synchronize()
        peak[v] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    times = {v: [] for v in models}
    for _ in range(args.net_rounds):
        for v in models:
            times[v].append(events_us(lambda: one(v), args.net_iters) / 1e3)
    ms = {v: summary(t) for v, t in times.items()}
    return {"what": "VGG11 bf16 channels_last with own_vgg_conv, %d structured images at 224 x 224, forward + input gradient "
                    "of sum(logits^2); own_vgg_first_conv off (the parent's route: the yardstick) / on, alternating rounds "
                    "of %d passes" % (b, args.net_iters),
            "against_the_fp32_network_on_8_images": acc, "ms_per_pass": ms, "peak_allocated_mib": peak,
            "on_against_off": verdict(ms["on"], ms["off"])}


def markdown(doc):
    g, n = doc["group1"], doc["network"]
    cell = lambda s: "%.0f [%.0f .. %.0f]" % (s["median"], s["min"], s["max"])
    lines = ["# VGG11's first group on the fused kernels (`own_vgg_first_conv`)", "",
             "Written by `tools/bench_vgg_first_conv.py`; kernel source hash `%s`, %s.  One process, one run, alternating "
             "rounds, device events: that is what these figures can claim.  A route is called faster only where every one of "
             "its rounds is below every round of the other.  ASR and other boxes: not measured."
             % (doc["kernel_source_hash"], doc["device"]), "",
             "## Group 1 (3 -> 64 at 224 x 224, pooled), %d images (microseconds, median [min .. max] of %d rounds)"
             % (g["B"], doc["rounds"]), "",
             "| direction | fused | parent's route | fused is | byte bound at %.1f TB/s | share of the bound |" % FLAT_COPY_TB_S,
             "|---|---|---|---|---|---|"]
    for d, name in (("fwd", "forward"), ("bwd", "input gradient")):
        lines.append("| %s | %s | %s | %s | %.0f | %.2f |" % (name, cell(g["us"]["fused_" + d]), cell(g["us"]["parent_" + d]),
                                                            g["fused_against_parent"][d], g["byte_bound"]["us_at_flat_copy_rate"],
                                                            g["share_of_byte_bound_at_median"][d]))
    lines += ["", "Algorithmic bytes per direction: image %.0f MB + pooled tensor %.0f MB + index %.0f MB = %.0f MB."
              % tuple(g["byte_bound"][k] / 1e6 for k in ("image", "pooled", "idx", "total")), "",
              "## Whole network", "", n["what"] + ".", ""]
    for v in ("off", "on"):
        s = n["ms_per_pass"][v]
        lines.append("- switch %s: %.2f ms median [%.2f .. %.2f], peak allocated %.0f MiB"
                     % (v, s["median"], s["min"], s["max"], n["peak_allocated_mib"][v]))
    lines += ["- on against off: %s" % n["on_against_off"], ""]
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_first_conv_bench.json"))
    args = p.parse_args()
    if args.rounds < 5 or args.net_rounds < 5:
        raise SystemExit("at least 5 alternating rounds")
    dev = torch.device("cuda", 0)
    models = build(dev)
    doc = {"what": "own_vgg_first_conv on against off (own_vgg_conv on in both), one process, alternating rounds, device events; "
                   "microseconds per call in `group1`, milliseconds per pass in `network`",
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters}
    doc["group1"] = bench_group(args, dev, models)
    print(json.dumps(doc["group1"]), flush=True)
    doc["network"] = bench_network(args, dev, models)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(markdown(doc) + "\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
