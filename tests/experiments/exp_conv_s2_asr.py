"""Experiment: the protocol of experiment 6 (exp_asr_gap6.py: FusedResNet-50 bf16, learn 300 steps on 512 structured
images, DDrague attack on held-out images, fp32 judge, same seeds) with a THIRD variant:
  default   the three stride-2 3x3 convolutions in bf16 through the library
  s2_fp32   the same three convolutions in fp32 through the library (bf16-valued input / weight widened, result rounded
            to bf16 once), forward and through autograd backward — 1/16 of the matrix pipe's bf16 rate
  own       FusedResNet(own_strided_conv=True): adil_conv3x3_s2_fwd / _bwd (bf16 MFMA, fp32 accumulation, one rounding)
and, on one batch, the outputs and input gradients of the three layers, own against s2_fp32: products of two bf16 values
are exact in fp32, so the two differ by fp32 summation order only, i.e. by a rare one-ulp flip of the bf16 result.
Environment: T (learning steps, 300), S (inference steps, 100), N_EVAL (4096), BS (512), SEEDS ("6033"), VARIANTS.
Prints one JSON object."""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import torch
import torch.nn.functional as F

from attacks import ADIL
from dl_attack_on_imagenet_amd import engine, zoo
from oracle import adil_oracle as O
from structured import fit_centroid_head, structured_images

n, k, eps, dev = 512, 50, 8 / 255, "cuda"
T, S = int(os.environ.get("T", 300)), int(os.environ.get("S", 100))
n_eval, bs = int(os.environ.get("N_EVAL", 4096)), int(os.environ.get("BS", 512))
seeds = [int(s) for s in os.environ.get("SEEDS", "6033").split(",") if s]          # SEEDS="": the layer comparison alone
variants = os.environ.get("VARIANTS", "default,s2_fp32,own").split(",")
out = {"T": T, "S": S, "n_eval": n_eval, "device": torch.cuda.get_device_name(0)}
images, labels = structured_images(n, 10, seed=3)
held, held_labels = structured_images(n_eval, 10, seed=3, draw=1)
tmp = tempfile.mkdtemp()
ref = zoo.build_classifier("resnet50", seed=0, device=dev)
fit_centroid_head(ref, images, labels, 10, dev, target_margin=10.0)
path = os.path.join(tmp, "fitted.pt")
torch.save(ref[-1].state_dict(), path)
ref = zoo.build_classifier("resnet50", seed=0, weights=path, device=dev)
kw = dict(seed=0, weights=path, device=dev, dtype=torch.bfloat16, channels_last=True, fuse_bn_act=True, fuse_stem=True)
lab0 = torch.zeros(bs, dtype=torch.long, device=dev)


def strided_layers(model):
    return [m for m in model.modules() if isinstance(m, zoo._ConvAffine) and m.conv.kernel_size == (3, 3) and m.conv.stride == (2, 2)]


def widen_stride2(model):
    """The three stride-2 3x3 convolutions of the fused network in fp32 (exp_asr_gap6.widen_stride2)."""
    for mod in strided_layers(model):
        conv = mod.conv
        w32 = conv.weight.detach().float()

        def raw(x, conv=conv, w32=w32):
            return F.conv2d(x.float(), w32, None, conv.stride, conv.padding).to(x.dtype).contiguous(memory_format=torch.channels_last)
        mod.raw_conv = raw
    return len(strided_layers(model))


def build(variant):
    net = zoo.build_classifier("resnet50", own_strided_conv=(variant == "own"), **kw)
    if variant == "s2_fp32":
        assert widen_stride2(net) == 3
    return net


def ulps(a, b):
    """|a - b| of two bf16 tensors in units of the larger one's last place."""
    a32, b32 = a.float(), b.float()
    big = torch.maximum(a32.abs(), b32.abs()).clamp_min(2.0 ** -126)
    return (a32 - b32).abs() / torch.exp2(torch.floor(torch.log2(big)) - 7)


def layer_comparison():
    """Own kernel against the fp32-widened library call, layer by layer, on the activations of one real batch."""
    own, wide = build("own"), build("s2_fp32")
    rows, inputs = [], []
    for m in strided_layers(own):                        # record what each layer is fed in a real forward pass
        def rec(x, orig=m.raw_conv):
            inputs.append(x.detach())
            return orig(x)
        m.raw_conv = rec
    with torch.no_grad():
        own(images[:64].to(dev).to(torch.bfloat16))
    for m in strided_layers(own):
        del m.raw_conv
    for lo, lw, x in zip(strided_layers(own), strided_layers(wide), inputs):
        c = lo.conv.in_channels
        xo, xw = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        yo, yw = lo.raw_conv(xo), lw.raw_conv(xw)
        g = torch.randn(yo.shape, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        (go,) = torch.autograd.grad(yo, xo, g)
        (gw,) = torch.autograd.grad(yw, xw, g)
        rows.append({"C": c, "N": lo.conv.out_channels, "H": x.shape[2], "W": x.shape[3],
                     "fwd": flips(yo.detach(), yw.detach()), "bwd": flips(go, gw.to(torch.bfloat16))})
    return rows


def flips(a, b):
    """How two bf16 results of the same fp32-exact products differ: the fraction of elements with different bits, the
    fraction more than one bf16 ulp apart, and for those (fp32 summation noise is absolute, so it spans several ulps only
    of a result that cancelled to near zero) their largest magnitude and difference, in units of the tensor's rms."""
    u = ulps(a, b)
    rms = float(b.float().square().mean().sqrt())
    far = u > 1
    big = torch.maximum(a.float().abs(), b.float().abs())
    return {"differing_fraction": float((u > 0).float().mean()), "more_than_one_ulp_fraction": float(far.float().mean()),
            "rms": rms, "max_abs_diff_over_rms": float((a.float() - b.float()).abs().max()) / rms,
            "largest_value_more_than_one_ulp_apart_over_rms": float(big[far].max()) / rms if bool(far.any()) else 0.0}


@torch.no_grad()
def fooled(net, x, adv):
    return int((net(adv).argmax(-1) != net(x).argmax(-1)).sum())


def pipeline(net, seed, name):
    g = torch.Generator().manual_seed(seed)
    d0 = -1 + 2 * torch.rand(3, 224, 224, k, generator=g)
    v0 = O.project_onto_l1_ball(torch.rand(n, k, generator=g), eps)
    x16, index = images.to(dev).to(torch.bfloat16), torch.arange(n, device=dev)
    lab = engine.predict(net, x16)
    learner = engine.DictionaryLearner(d0.to(dev), v0.to(dev), eps, 0.01, "logits", False, 50.0)
    t0 = time.time()
    for it in range(T):
        learner.step(net, x16, index, lab)
        if it % 50 == 49:
            torch.cuda.synchronize()
            print(f"  {name}: learning iteration {it + 1}, {(time.time() - t0) / (it + 1) * 1e3:.2f} ms per step so far", file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / T * 1e3
    torch.save([learner.d.cpu(), learner.v.cpu(), [], [], torch.tensor(0.)], os.path.join(tmp, f"ImageNet_{name}.bin"))
    atk = ADIL(net, eps=eps, n_atoms=k, attack="supervised", model_name=name, loss="logits", steps_inference=S, dict_dir=tmp,
               stream_dtype=torch.bfloat16)
    f32 = 0
    for lo in range(0, n_eval, bs):
        x = held[lo:lo + bs].to(dev).to(torch.bfloat16)
        adv = atk(x, lab0[:x.shape[0]])
        f32 += fooled(ref, x.float(), adv.float())
        print(f"  {name}: attacked {lo + bs} images, fooled {f32}", file=sys.stderr, flush=True)
    return f32 / n_eval, ms


out["layers_own_vs_s2_fp32"] = layer_comparison()
print(json.dumps(out["layers_own_vs_s2_fp32"]), file=sys.stderr, flush=True)
out["runs"] = []
for seed in seeds:
    rec = {"seed": seed}
    for v in variants:
        print(f"seed {seed}: {v} ...", file=sys.stderr, flush=True)
        net = build(v)
        rec[v], rec[v + "_learn_ms_per_step"] = pipeline(net, seed, f"{v}{seed}")
        del net
    out["runs"].append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)
print(json.dumps(out))
