"""VGG11's eight groups conv3x3 + bias + ReLU [+ 2x2 max-pool] on the hand-written kernels (`own_vgg_conv`: adil_conv3x3 /
adil_conv3x3_wide, adil_bias_relu_pool2_fwd / _bwd, adil_affine_act) against the library route they replace (Conv2d, ReLU,
MaxPool2d modules on channels_last bf16 tensors and their autograd), timed in ONE process, alternating, every shape warmed
up, with device events:
  (a) per group at 224 x 224 and --batch images: forward (with the autograd graph recorded, as the attack runs it) and input
      gradient, medians and the library's own round-to-round spread, FLOP/s and algorithmic bytes from the shapes;
  (b) a whole bf16 VGG11 forward + input gradient of sum(logits^2), switch off (the code path as it was: the yardstick)
      against on, in alternating rounds, with the peak allocated memory of a pass.
"Faster" is claimed for a group or for the network only where EVERY switch-on round is below EVERY switch-off round.
Writes profiles/vgg_conv_bench.json and profiles/vgg_conv_bench.md and prints the JSON.

usage: python tools/bench_vgg_conv.py [--batch 256] [--rounds 5] [--iters 5] [--net-rounds 5] [--net-iters 2] [--out PATH]
       --only layers|network restricts the run"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from bench_depthwise import events_us, forward_and_gradient, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

BF16 = torch.bfloat16


def network_groups():
    """(C, N, H = W, pooled) of the eight groups at 224 x 224, from the network itself."""
    feats = zoo._OwnVggFeatures(zoo.VGG11(num_classes=8).features)
    out, h = [], 224
    for conv_name, _, pool_name in feats._groups:
        conv = feats._modules[conv_name]
        out.append((conv.in_channels, conv.out_channels, h, pool_name is not None))
        h = h // 2 if pool_name else h
    return out


def summary(ts):
    s = sorted(ts)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2),
            "spread": round(s[-1] - s[0], 2), "rounds": [round(t, 2) for t in ts]}


def bench_layers(args, dev):
    out, b = [], args.batch
    for i, (c, n, hw, pooled) in enumerate(network_groups()):
        gen = torch.Generator().manual_seed(100 + i)
        conv = nn.Conv2d(c, n, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (2.0 / (9 * n)) ** 0.5)
            conv.bias.copy_(torch.randn(n, generator=gen) * 0.1)
        bias32 = conv.bias.detach().clone().to(dev)
        conv = conv.to(dev, BF16).to(memory_format=torch.channels_last).requires_grad_(False)
        relu, pool = nn.ReLU(inplace=True), nn.MaxPool2d(2, 2)
        x = torch.randn(b, hw, hw, c, generator=gen).bfloat16().to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        oh = hw // 2 if pooled else hw
        g = torch.randn(b, oh, oh, n, generator=gen).bfloat16().to(dev).permute(0, 3, 1, 2)
        ones = torch.ones(n, device=dev)
        packed = c % 64 == 0
        if packed:
            wf, wb = (t.to(dev) for t in ops.pack_conv3x3_weights(conv.weight))

        def lib_fwd():
            y = relu(conv(x))
            return pool(y) if pooled else y

        def own_fwd():
            if not packed:                                          # the first convolution stays the module it is
                return ops.bias_relu_pool2(conv(x), None)
            raw = ops.conv3x3(x, wf, wb) if hw <= 63 else ops.conv3x3_wide(x, wf, wb)
            return ops.bias_relu_pool2(raw, bias32) if pooled else ops.affine_act(raw, ones, bias32, relu=True)

        keep = {"lib": lib_fwd(), "own": own_fwd()}
        fns = {"own_fwd": own_fwd, "lib_fwd": lib_fwd,
               "own_bwd": lambda: torch.autograd.grad(keep["own"], x, g, retain_graph=True),
               "lib_bwd": lambda: torch.autograd.grad(keep["lib"], x, g, retain_graph=True)}
        for fn in fns.values():                                                                 # library find / warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        df = float((keep["own"].float() - keep["lib"].float()).abs().max())
        db = float((fns["own_bwd"]()[0].float() - fns["lib_bwd"]()[0].float()).abs().max())
        times = {key: [] for key in fns}
        for _ in range(args.rounds):
            for key, fn in fns.items():
                times[key].append(events_us(fn, args.iters))
        us = {key: summary(t) for key, t in times.items()}
        m = b * hw * hw
        flop = 2.0 * m * 9 * c * n
        # what the own route moves at the least: the convolution reads x and writes raw; the epilogue reads raw and writes
        # the (pooled) output and, where pooled, one index byte per output; the gradient runs the same tensors backwards
        conv_bytes = 2.0 * m * (c + n)
        epi_bytes = 2.0 * m * n * (1 + 0.25) + m * n / 4 if pooled else 2.0 * m * n * 2
        if not packed:
            epi_bytes = 2.0 * m * n * (1 + 0.25) + m * n / 4
        for key in us:
            us[key]["tflop_per_s_at_median"] = round(flop / us[key]["median"] / 1e6, 1)
        verdict = {}
        for d in ("fwd", "bwd"):
            o, lb = us["own_" + d], us["lib_" + d]
            verdict[d] = ("faster" if o["max"] < lb["min"] else "slower" if o["min"] > lb["max"] else "not separated")
        out.append({"group": i + 1, "C": c, "N": n, "H": hw, "W": hw, "B": b, "pooled": pooled,
                    "convolution": "library" if not packed else "adil_conv3x3" if hw <= 63 else "adil_conv3x3_wide",
                    "gflop": round(flop / 1e9, 1), "conv_mbytes": round(conv_bytes / 1e6, 1),
                    "epilogue_mbytes": round(epi_bytes / 1e6, 1),
                    "max_abs_diff_own_vs_library": {"fwd": df, "bwd": db}, "us": us, "own_against_library": verdict})
        print(json.dumps(out[-1]), flush=True)
        del keep, fns, x, g, conv
        torch.cuda.empty_cache()
    tot = {key: round(sum(r["us"][key]["median"] for r in out) / 1e3, 3) for key in ("own_fwd", "lib_fwd", "own_bwd", "lib_bwd")}
    return {"groups": out, "ms_summed_at_median": tot,
            "groups_that_are_not_faster": [(r["group"], d, r["own_against_library"][d]) for r in out for d in ("fwd", "bwd")
                                           if r["own_against_library"][d] != "faster"]}


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    kw = dict(seed=0, device=dev)
    models = {v: zoo.build_classifier("vgg11", dtype=BF16, channels_last=True, own_vgg_conv=(v == "on"), **kw)
              for v in ("off", "on")}
    out = {"what": "VGG11 bf16 channels_last, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); "
                   "own_vgg_conv off (the code path as it was: the yardstick) / on, alternating rounds of %d passes"
                   % (b, args.net_iters)}
    ref = zoo.build_classifier("vgg11", **kw)
    xs = images[:8].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    acc = {}
    for v, model in models.items():
        lg, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((lg - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_8_images"] = {"rms_logit": float(lr.square().mean().sqrt()), **acc}
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
    out["ms_per_pass"] = {v: summary(t) for v, t in times.items()}
    out["peak_allocated_mib"] = peak
    d, w = out["ms_per_pass"]["off"], out["ms_per_pass"]["on"]
    out["switch_on_against_off"] = {"gain_ms_at_median": round(d["median"] - w["median"], 3),
                                    "larger_spread_ms": max(d["spread"], w["spread"]),
                                    "every_on_round_beats_every_off_round": bool(w["max"] < d["min"])}
    return out


def markdown(doc):
    lines = ["# VGG11 on the own 3x3 / bias + ReLU + pool kernels (`own_vgg_conv`)", "",
             "Written by `tools/bench_vgg_conv.py`; kernel source hash `%s`, %s.  One process, alternating rounds, device "
             "events.  A route is called faster only where every one of its rounds is below every round of the other."
             % (doc["kernel_source_hash"], doc["device"]), ""]
    if "layers" in doc:
        lines += ["## Per group, %d images at 224 x 224 (microseconds, median [min .. max] of %d rounds)"
                  % (doc["layers"]["groups"][0]["B"], doc["rounds"]), "",
                  "| group | shape | convolution | own fwd | library fwd | fwd | own bwd | library bwd | bwd | own conv-FLOP/s fwd |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        cell = lambda s: "%.0f [%.0f .. %.0f]" % (s["median"], s["min"], s["max"])
        for r in doc["layers"]["groups"]:
            u = r["us"]
            lines.append("| %d | %d -> %d at %d%s | %s | %s | %s | %s | %s | %s | %s | %.0f T |" % (
                r["group"], r["C"], r["N"], r["H"], ", pooled" if r["pooled"] else "", r["convolution"], cell(u["own_fwd"]),
                cell(u["lib_fwd"]), r["own_against_library"]["fwd"], cell(u["own_bwd"]), cell(u["lib_bwd"]),
                r["own_against_library"]["bwd"], u["own_fwd"]["tflop_per_s_at_median"]))
        t = doc["layers"]["ms_summed_at_median"]
        lines += ["", "Summed at the medians: forward own %.2f ms / library %.2f ms, input gradient own %.2f ms / library %.2f ms."
                  % (t["own_fwd"], t["lib_fwd"], t["own_bwd"], t["lib_bwd"]),
                  "Not faster: %s." % (doc["layers"]["groups_that_are_not_faster"] or "none"), ""]
    if "network" in doc:
        n = doc["network"]
        lines += ["## Whole network", "", n["what"] + ".", ""]
        for v in ("off", "on"):
            s = n["ms_per_pass"][v]
            lines.append("- switch %s: %.2f ms median [%.2f .. %.2f], peak allocated %.0f MiB"
                         % (v, s["median"], s["min"], s["max"], n["peak_allocated_mib"][v]))
        lines += ["- every switch-on round below every switch-off round: %s"
                  % n["switch_on_against_off"]["every_on_round_beats_every_off_round"], ""]
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=2)
    p.add_argument("--only", choices=["layers", "network"], default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_conv_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    doc = {"what": "own_vgg_conv route vs the library route (Conv2d + ReLU [+ MaxPool2d] modules, channels_last bf16, autograd), "
                   "one process, alternating rounds, device events; microseconds per call in `layers`, milliseconds per pass in "
                   "`network`",
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters}
    if args.only != "network":
        doc["layers"] = bench_layers(args, dev)
    if args.only != "layers":
        doc["network"] = bench_network(args, dev)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".md", "w") as f:
        f.write(markdown(doc) + "\n")
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
