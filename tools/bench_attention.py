"""The whole-head attention kernels (adil_attn_fwd / adil_attn_bwd) against the torch statements of
`zoo._EncoderBlock._attention` between the two projections (reshape + permute, q k^T, softmax, p v, permute + reshape, under
autograd).  Timed in ONE process, alternating, warmed up, with device events:
  (a) the segment alone, qkv -> o forward and go -> gqkv backward, at B = 512, T = 197, H = 12; for the two kernels also
      algorithmic bytes / time over the 5.1 TB/s copy yardstick (profiles/r04_stream_patterns.md; forward: qkv + o + lse,
      backward: qkv + o + go + gqkv + lse);
  (b) a whole forward + input gradient of ViT-B/16 in bf16 at 512 images, `own_attention` off against on;
  (c) torch.cuda.max_memory_allocated of (b) for both.
Writes one JSON document (default profiles/attention_bench.json) and prints it.

usage: python tools/bench_attention.py [--batch 512] [--rounds 7] [--iters 5] [--net-rounds 5] [--net-iters 1] [--out PATH]
       --only kernels|network restricts the run"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bench_depthwise import events_us, forward_and_gradient, stats, structured_batch  # noqa: E402
from dl_attack_on_imagenet_amd import _lib, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402

COPY_TB_PER_S = 5.1


def torch_segment(qkv, heads):
    """The statements of `_attention` between the two F.linear calls."""
    b, t, dim3 = qkv.shape
    hd = dim3 // 3 // heads
    x = qkv.reshape(b, t, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    w = torch.softmax((q @ k.transpose(-1, -2)) * (hd ** -0.5), dim=-1)
    return (w @ v).permute(0, 2, 1, 3).reshape(b, t, heads * hd)


def bench_kernels(args, dev):
    lib = _lib.load()
    b, t, h = args.batch, 197, 12
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn(b, t, 3 * h * 64, generator=gen).bfloat16().to(dev)
    go = torch.randn(b, t, h * 64, generator=gen).bfloat16().to(dev)
    o = torch.empty(b, t, h * 64, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(b, h, t, dtype=torch.float32, device=dev)
    gqkv = torch.empty_like(qkv)
    qt = qkv.clone().requires_grad_(True)
    yt = torch_segment(qt, h)
    st, P = ops._stream(), ops._ptr
    fns = {
        "own_fwd": lambda: lib.adil_attn_fwd(P(qkv), P(o), P(lse), b, t, h, st),
        "torch_fwd": lambda: torch_segment(qt.detach(), h),
        "own_bwd": lambda: lib.adil_attn_bwd(P(qkv), P(o), P(lse), P(go), P(gqkv), b, t, h, st),
        "torch_bwd": lambda: torch.autograd.grad(yt, qt, go, retain_graph=True),
    }
    for fn in fns.values():                                                                      # library find / warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    (gt,) = torch.autograd.grad(yt, qt, go, retain_graph=True)
    agree = {"relative_diff_o_own_vs_torch": float((o.float() - yt.detach().float()).norm() / yt.detach().float().norm()),
             "relative_diff_gqkv_own_vs_torch": float((gqkv.float() - gt.float()).norm() / gt.float().norm())}
    times = {key: [] for key in fns}
    for _ in range(args.rounds):
        for key, fn in fns.items():
            times[key].append(events_us(fn, args.iters))
    e_qkv, e_o, e_lse = float(b) * t * 3 * h * 64 * 2, float(b) * t * h * 64 * 2, float(b) * h * t * 4
    nbytes = {"own_fwd": e_qkv + e_o + e_lse, "own_bwd": 2 * e_qkv + 2 * e_o + e_lse}
    us = {key: stats(ts, nbytes.get(key)) for key, ts in times.items()}
    for key in nbytes:
        us[key]["fraction_of_copy_yardstick"] = round(us[key]["algorithmic_tb_per_s_at_median"] / COPY_TB_PER_S, 3)
    own = [f + g for f, g in zip(times["own_fwd"], times["own_bwd"])]
    ref = [f + g for f, g in zip(times["torch_fwd"], times["torch_bwd"])]
    seg = {"own": stats(own), "torch": stats(ref)}
    spread = seg["torch"]["max"] - seg["torch"]["min"]
    margin = seg["torch"]["median"] - seg["own"]["median"]
    out = {"B": b, "T": t, "H": h, "algorithmic_mbytes": {k: round(v / 1e6, 1) for k, v in nbytes.items()}, **agree, "us": us,
           "segment_fwd_plus_bwd_us": seg,
           "torch_spread_between_rounds_us": round(spread, 2), "margin_us_at_median": round(margin, 2),
           "ratio_torch_over_own_at_median": round(seg["torch"]["median"] / seg["own"]["median"], 2),
           "condition": {"own_faster_than_torch_by_more_than_the_torch_spread": margin > spread}}
    print(json.dumps(out), flush=True)
    return out


def bench_network(args, dev):
    b = args.batch
    images = structured_batch(b)
    kw = dict(seed=0, device=dev)
    models = {"off": zoo.build_classifier("vit_b_16", dtype=torch.bfloat16, **kw),
              "on": zoo.build_classifier("vit_b_16", dtype=torch.bfloat16, own_attention=True, **kw)}
    out = {"what": "ViT-B/16 bf16, %d structured images at 224 x 224, forward + input gradient of sum(logits^2); own_attention off "
                   "(plain matmuls and softmax) / on (the attention kernels); alternating rounds of %d passes" % (b, args.net_iters)}
    ref = zoo.build_classifier("vit_b_16", **kw)
    xs = images[:16].to(dev)
    lr, gr = forward_and_gradient(ref, xs)
    rms = float(lr.square().mean().sqrt())
    acc = {}
    for v, model in models.items():
        l, g = forward_and_gradient(model, xs.bfloat16())
        acc[v] = {"mean_abs_logit_error": float((l - lr).abs().mean()),
                  "input_gradient_relative_error": float((g - gr).norm() / gr.norm())}
    out["against_the_fp32_network_on_16_images"] = {"rms_logit": rms, **acc}
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
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        one(v)
        torch.cuda.synchronize()
        peak[v] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 3)
    out["peak_allocated_gib"] = peak
    times = {v: [] for v in models}
    for _ in range(args.net_rounds):
        for v in models:
            times[v].append(events_us(lambda: one(v), args.net_iters) / 1e3)
    out["ms_per_pass"] = {v: {"median": round(sorted(ts)[len(ts) // 2], 3), "min": round(min(ts), 3), "max": round(max(ts), 3),
                              "spread": round(max(ts) - min(ts), 3), "rounds": [round(u, 3) for u in ts]} for v, ts in times.items()}
    off, on = out["ms_per_pass"]["off"], out["ms_per_pass"]["on"]
    out["condition"] = {"on_no_slower_than_off_at_median": on["median"] <= off["median"],
                        "difference_ms_at_median": round(on["median"] - off["median"], 3)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--net-rounds", type=int, default=5)
    p.add_argument("--net-iters", type=int, default=1)
    p.add_argument("--only", choices=["kernels", "network"], default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    out = {"what": "adil_attn_fwd / _bwd vs the torch statements of zoo._EncoderBlock._attention between the two projections "
                   "(autograd), one process, alternating rounds, device events; microseconds per call; fractions are algorithmic "
                   "bytes / time over the %.1f TB/s copy yardstick" % COPY_TB_PER_S,
           "kernel_source_hash": source_hash(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
           "iters_per_round": args.iters, "attn_max_tokens": ops.attention_max_tokens()}
    if args.only != "network":
        out["kernels"] = bench_kernels(args, dev)
    if args.only != "kernels":
        out["network"] = bench_network(args, dev)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
