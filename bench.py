"""ADiL hot-path benchmark (driver contract: `python bench.py --gpus N --steps K --warmup W`, one JSON line).

Workload = BASELINE.json configs[1]: ADiL vs ResNet-50, 512 images per GPU, 50 atoms, bf16 image streams.
A "step" is ONE pass of the learning hot path over one batch (the loop body of learn_dictionary_a,
adil.py:168-191): clean pseudo-label forward, perturbation synthesis x + D v, classifier forward + backward,
grad_d / grad_v in one pass over dLoss/dx, AdamW(D)+clamp, AdamW(all rows of V)+l1-ball projection, and for
N > 1 one RCCL all-reduce(SUM) of grad_d.  The default K = 100 steps are the config's "100 inner iters".
Every step synthesises and evaluates B adversarial images per GPU, so value = N*B*K / seconds.
Inputs are synthetic (seeded U[0,1) images, seeded random-init ResNet-50) and resident in HBM before timing.

A plain run sets up, warms up, times the steps and prints the headline line, nothing else.  `--full` adds the other
measurements to the JSON line: `roofline` for the dominant hand-written kernel (HIP events recorded on the launch stream
inside the timed region; algorithmic bytes per launch from DESIGN.md), per-kernel times, the learn mode's other
pseudo-label policy timed over as many steps again, and `cpu_baseline` (the CPU oracle timed on a bounded sample of the
same workload on the host cores; rank 0, N = 1 only).

`--dump-outputs DIR` writes what the timed path computed in its last step as DIR/<name>.npy (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=None, help="timed steps (default: 100; --mode transfer: 4 batches)")
    p.add_argument("--warmup", type=int, default=None, help="untimed steps (default: 5; --mode transfer: 1 batch)")
    p.add_argument("--mode", default="learn", choices=["learn", "inference", "transfer"],
                   help="learn: one step = the loop body of learn_dictionary_a (the headline, configs[1]); inference: one "
                        "step = one iteration of forward_supervised_DDrague over the batch; transfer: configs[3] as the "
                        "workload it is — one step = one batch through performance.get_transfer_performance: the full "
                        "attack(x, y) (--steps-inference DDrague iterations with the stop test) against --model, then the six "
                        "classifiers of the reference CLI scored on the adversary")
    p.add_argument("--model", default="resnet50")
    p.add_argument("--batch", type=int, default=512, help="images per GPU (weak scaling)")
    p.add_argument("--atoms", type=int, default=None, help="dictionary atoms (default 50 = configs[1]; --mode transfer: 100, the "
                                                           "reference's n_atoms, demo_dL_attack.py:88,114)")
    p.add_argument("--steps-inference", type=int, default=100, help="--mode transfer: DDrague iterations per attack call "
                                                                    "(demo_dL_attack.py:186 default)")
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--loss", default="logits", choices=["logits", "ce"])
    p.add_argument("--channels-last", type=int, default=1)
    p.add_argument("--fold-bn", type=int, default=1,
                   help="fold the frozen classifier's eval-mode BatchNorms into its convolutions (same function)")
    p.add_argument("--fuse-bn-act", type=int, default=1,
                   help="ResNets: run eval-BatchNorm + residual + ReLU as one epilogue kernel per convolution "
                        "(zoo.FusedResNet; conv weights untouched; supersedes --fold-bn)")
    p.add_argument("--fuse-stem", type=int, default=1,
                   help="ResNets with --fuse-bn-act, bf16: Normalize + conv1 + bn1 + ReLU + maxpool (forward and input "
                        "gradient) as the hand-written stem kernels (csrc/adil_stem.hip)")
    p.add_argument("--pad-cin", type=int, default=8,
                   help="zero-pad the first conv's 3 input channels to this width (0 = off); see zoo.ChannelPaddedConv")
    p.add_argument("--cache-labels", type=int, default=1,
                   help="1 (default since round 3, = ADIL's default): the clean pseudo-label of an image is computed on its "
                        "first visit and reused (engine.LabelCache; measured result-neutral, profiles/r03_label_stability.md); "
                        "0: the reference's op sequence, which recomputes it in every step (adil.py:172, quirk Q4).  The "
                        "other variant is timed as well and reported in `config`")
    p.add_argument("--fp8-synth", type=int, default=0,
                   help="1: the D.V contraction of the synthesis on fp8 (e4m3) MFMAs (BASELINE.json configs[4]); learn mode")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline does not need: kernel brackets and roofline, the other pseudo-label "
                        "policy (learn mode), the collective's brackets, the CPU baseline")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                        "(learn: d, v, loss, fooled; inference: adversarial_images, codes; transfer: fooling_rate, rmse, mse "
                        "per target in the order of TRANSFER_TARGETS); at most 60 MB in all, larger arrays as a fixed sample")
    p.add_argument("--cpu-baseline", type=int, default=1, help="with --full: time the CPU oracle as well")
    p.add_argument("--cpu-batch", type=int, default=48, help="images of the config-2-shape CPU sample (48 images x 1 step per "
                                                             "pseudo-label policy: ~12 + ~18 s on the box's host cores)")
    p.add_argument("--cpu-steps", type=int, default=1)
    p.add_argument("--cpu-config1", type=int, default=1, help="also run configs[0] (resnet18, 32 images, 10 atoms, 20 "
                                                              "iterations, fp32) in full on the host cores and on the GPU")
    a = p.parse_args()
    transfer = a.mode == "transfer"
    a.steps = a.steps if a.steps is not None else (4 if transfer else 100)
    a.warmup = a.warmup if a.warmup is not None else (1 if transfer else 5)
    a.atoms = a.atoms if a.atoms is not None else (100 if transfer else 50)
    return a


class KernelTimer:
    """Brackets every launch group of the hand-written kernels with HIP events on the launch stream."""

    GROUPS = ("pack_codes", "synth", "grad", "adamw_clamp_", "adamw_l1ball_", "zstep_", "zstep_codes_")

    def __init__(self, ops):
        self.ops, self.enabled, self.records, self.empty = ops, False, {}, []
        for name in self.GROUPS:
            setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def timed(*a, **k):
            if not self.enabled:
                return fn(*a, **k)
            key = name
            if name == "grad" and a[0].dtype == torch.float32 and not k.get("want_d", True):
                key = "grad[z D_dagger^T]"                        # the fp32-z contraction of the DDrague iteration
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.records.setdefault(key, []).append((e0, e1))
            if name == "synth":                                  # an EMPTY bracket, recorded the same way on the same
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)   # stream: what
                c0.record()                                      # two back-to-back event markers cost by themselves
                c1.record()
                self.empty.append((c0, c1))
            return out
        return timed

    def empty_bracket_ms(self):
        return sum(a.elapsed_time(b) for a, b in self.empty) / len(self.empty) if self.empty else 0.0

    def summary_ms(self, calibrated=False):
        """Mean bracket time per launch group (this is what the JSON reports: it agrees with rocprofv3's kernel
        duration to a few %, see profiles/).  `calibrated` subtracts the mean empty-bracket time — reported only as
        a bound on what the event markers themselves may contribute."""
        off = self.empty_bracket_ms() if calibrated else 0.0
        out = {}
        for name, evs in self.records.items():
            if evs:
                out[name] = max(sum(a.elapsed_time(b) for a, b in evs) / len(evs) - off, 0.0)
        return out


DUMP_BYTES = 60 * 10 ** 6      # --dump-outputs: all arrays together


def dump_outputs(path, arrays):
    """Write every array of `arrays` as path/<name>.npy: float64 stays float64, everything else becomes float32.  The
    arrays are taken smallest first, and one that is larger than its even share of what DUMP_BYTES has left is written as
    a flat sample of its elements instead: indices drawn from a generator seeded with 0 and sorted, so that two runs (two
    builds) at the same arguments sample the same elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    items = sorted(((name, torch.as_tensor(a).detach()) for name, a in arrays.items()), key=lambda kv: kv[1].numel())
    left = DUMP_BYTES
    for i, (name, a) in enumerate(items):
        a = a.to(torch.float64 if a.dtype == torch.float64 else torch.float32)
        share = left // (len(items) - i)
        if a.numel() * a.element_size() > share:
            n = share // a.element_size()
            idx = torch.randint(a.numel(), (n,), generator=torch.Generator().manual_seed(0)).sort().values
            a = a.reshape(-1)[idx.to(a.device)]
        a = a.cpu()
        left -= a.numel() * a.element_size()
        np.save(os.path.join(path, name + ".npy"), a.numpy())


def algorithmic_bytes(B, P, K, N, s, mode="learn"):
    """Per launch group, SURVEY.md §8(d): s = bytes/element of the image streams, D / V master fp32."""
    if mode == "inference":                                        # one DDrague iteration: 7*B*P*4 + 3*B*P*s + 4*P*K*4
        return {
            "grad[z D_dagger^T]": B * P * 4 + P * K * 4 + B * K * 4,   # read z (fp32), read D_dagger, write codes
            "synth": 2 * B * P * s + P * K * 4 + B * K * 4,            # read x, write x + D v, read D
            "grad": B * P * s + P * K * 4 + B * K * 4,                 # read g, read D, write dL/dv
            "zstep_": 6 * B * P * 4 + P * K * 4 + B * K * 4,           # z, m, s read + written; D_dagger; dL/dv
            # round 4: the z-step that also produces the next iteration's codes (adil_zstep_codes): the same streams — the
            # contraction's own pass over z and D_dagger ("grad[z D_dagger^T]" above) is what the fusion removes, so it is
            # NOT credited here — plus the codes it writes
            "zstep_codes_": 6 * B * P * 4 + P * K * 4 + 2 * B * K * 4,
            "pack_codes": 2 * B * K * 4,
        }
    return {
        "synth": 2 * B * P * s + P * K * 4 + B * K * 4,            # read x, write x+Dv, read D (+ codes)
        "grad": B * P * s + P * K * 4 + P * K * 4 + B * K * 8,     # read g, read D, write grad_d (+ codes, grad_v)
        "adamw_clamp_": 7 * P * K * 4,                             # read p,g,m,s; write p,m,s
        "adamw_l1ball_": 7 * N * K * 4 + B * K * 4,
        "pack_codes": 2 * B * K * 4,
    }


def _config1_problem():
    """BASELINE.json configs[0] / BASELINE.md §3: resnet18, N = B = 32 images of 3x224x224, 10 atoms, 20 iterations, fp32,
    eps 8/255, lr 0.01, kappa 50, loss 'logits'; seeded synthetic inputs."""
    from oracle import adil_oracle as O
    g = torch.Generator().manual_seed(21)
    n, k, eps = 32, 10, 8 / 255
    images = torch.rand(n, 3, 224, 224, generator=g)
    d0 = -1 + 2 * torch.rand(3, 224, 224, k, generator=g)
    v0 = O.project_onto_l1_ball(torch.rand(n, k, generator=g), eps)
    return images, d0, v0, eps


def cpu_config1(dev):
    """configs[0] in full: the CPU oracle on the host cores, and the HIP path on the same inputs and seeds; per-iteration
    fooled counts and the final attack success rate (performance.py:238-246) of both."""
    from oracle import adil_oracle as O
    from dl_attack_on_imagenet_amd import engine, zoo
    images, d0, v0, eps = _config1_problem()
    n, T = images.shape[0], 20
    index = torch.arange(n)
    cpu_model = zoo.build_classifier("resnet18", seed=5)
    d, v = d0.clone(), v0.clone()
    od, ov = O.AdamWState(d, 0.01), O.AdamWState(v, 0.01)
    fooled_cpu = []
    t0 = time.perf_counter()
    for _ in range(T):
        _, fl = O.learn_step_a(cpu_model, images, index, d, v, od, ov, eps, "logits", -1.0, 50.0)
        fooled_cpu.append(int(fl))
    cpu_s = time.perf_counter() - t0
    with torch.no_grad():
        adv = images + (v @ d.reshape(-1, d.shape[-1]).t()).reshape(images.shape)
        asr_cpu = float((cpu_model(adv).argmax(-1) != cpu_model(images).argmax(-1)).float().mean())
    gpu_model = zoo.build_classifier("resnet18", seed=5, device=dev)
    learner = engine.DictionaryLearner(d0.to(dev), v0.to(dev), eps, 0.01, "logits", False, 50.0)
    x, idx = images.to(dev), index.to(dev)
    engine.DictionaryLearner(d0.to(dev), v0.to(dev), eps, 0.01, "logits", False, 50.0).step(gpu_model, x, idx)   # library warm-up
    fooled_gpu = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(T):
        _, fl = learner.step(gpu_model, x, idx)
        fooled_gpu.append(fl)
    torch.cuda.synchronize()
    gpu_s = time.perf_counter() - t0
    fooled_gpu = [int(f) for f in fooled_gpu]
    # the same 20 iterations with the step replayed as ONE hipGraph launch (this configuration is launch-bound)
    graphed = engine.DictionaryLearner(d0.to(dev), v0.to(dev), eps, 0.01, "logits", False, 50.0)
    fooled_graph = []
    for _ in range(3):                                           # two eager warm-up steps + the capturing one
        fooled_graph.append(graphed.step_graphed(gpu_model, x, idx)[1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(T - 3):
        fooled_graph.append(graphed.step_graphed(gpu_model, x, idx)[1])
    torch.cuda.synchronize()
    graph_s = (time.perf_counter() - t0) * T / (T - 3)
    fooled_graph = [int(f) for f in fooled_graph]
    with torch.no_grad():
        vp = engine.ops.pack_codes(learner.v, None, n)
        adv = engine.ops.synth(x, learner.d, vp, n)
        asr_gpu = float((gpu_model(adv).argmax(-1) != gpu_model(x).argmax(-1)).float().mean())
    return {"workload": "configs[0]: resnet18, 32 images 3x224x224, 10 atoms, 20 iterations, fp32, in full",
            "cpu_images_per_sec": n * T / cpu_s, "cpu_seconds": cpu_s, "gpu_images_per_sec": n * T / gpu_s,
            "gpu_seconds": gpu_s, "gpu_hipgraph_images_per_sec": n * T / graph_s, "gpu_hipgraph_seconds": graph_s,
            "asr_cpu": asr_cpu, "asr_gpu": asr_gpu, "fooled_per_iteration_cpu": fooled_cpu,
            "fooled_per_iteration_gpu": fooled_gpu, "fooled_per_iteration_gpu_hipgraph": fooled_graph}


def cpu_baseline(args, P_shape, dev):
    """The oracle (op-for-op the reference's sequence) on the host cores, bounded sample of the bench workload:
    configs[1] shape (same classifier, atoms, image size, loss) on `--cpu-batch` of its images — images/sec is a
    per-image rate, so the sample scales to the full batch linearly in everything except the AdamW pass over D
    (7*P*K*4 bytes per step, independent of the batch).  Plus configs[0] in full with the ASR of both
    paths on the same inputs."""
    from oracle import adil_oracle as O
    from dl_attack_on_imagenet_amd import zoo
    threads = torch.get_num_threads()
    b, k = args.cpu_batch, args.atoms
    model = zoo.build_classifier(args.model, seed=0)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(b, *P_shape, generator=g)
    d = -1 + 2 * torch.rand(*P_shape, k, generator=g)
    if args.mode == "inference":
        O.forward_supervised_ddrague(model, x[:2], d, 8 / 255, 1, args.loss)            # warm-up (allocators, MKL)
        iters = max(2, args.cpu_steps)
        t0 = time.perf_counter()
        O.forward_supervised_ddrague(model, x, d, 8 / 255, iters, args.loss)
        dt = time.perf_counter() - t0
        what = (f"{iters} iterations of the CPU oracle's forward_supervised_ddrague (incl. the once-per-call Gram / "
                f"pseudo-inverse)")
        value = b * iters / dt
    else:
        v = O.project_onto_l1_ball(torch.rand(b, k, generator=g), 8 / 255)
        od, ov = O.AdamWState(d, 0.01), O.AdamWState(v, 0.01)
        index = torch.arange(b)
        O.learn_step_a(model, x[:2], index[:2], d, v, od, ov, 8 / 255, args.loss, -1.0, 50.0)   # warm-up
        # the CPU figure beside `value` follows the SAME pseudo-label policy as `value` (cached labels by
        # default: 1 forward + 1 backward per step; the labels are handed in, as engine.LabelCache does from an image's
        # second visit on), and the other policy — the reference's own sequence, recomputing them: 2 forwards + 1
        # backward — is timed right after it on the same sample
        with torch.no_grad():
            cached = model(x).argmax(dim=-1)
        timings = {}
        for policy in (("cached", "recomputed") if args.cache_labels else ("recomputed", "cached")):
            t0 = time.perf_counter()
            for _ in range(args.cpu_steps):
                O.learn_step_a(model, x, index, d, v, od, ov, 8 / 255, args.loss, -1.0, 50.0,
                               labels=cached if policy == "cached" else None)
            timings[policy] = time.perf_counter() - t0
        same, other = ("cached", "recomputed") if args.cache_labels else ("recomputed", "cached")
        dt = timings[same]
        what = (f"{args.cpu_steps} learning step(s) of the CPU oracle (oracle/adil_oracle.py learn_step_a) with the pseudo-labels "
                f"{'handed in (cached policy, 1 fwd + 1 bwd: the policy of `value`)' if args.cache_labels else 'recomputed (2 fwd + 1 bwd: the policy of `value`)'}"
                f"; the other policy ({other}) took {timings[other]:.1f} s on the same sample")
        value = b * args.cpu_steps / dt
        other_value = b * args.cpu_steps / timings[other]
        # "separately, seconds per step of the dictionary ops alone" — the reference's op sequence without
        # the classifier (synthesis, backward through the tensordot for a given dLoss/dx, AdamW on D and all code rows,
        # l1 projection, clamp) at the FULL batch of the workload; compare with `dictionary_path_ms_per_step` of the GPU
        bf = args.batch
        gen = torch.Generator().manual_seed(1)
        xf, gf = torch.rand(bf, *P_shape, generator=gen), torch.randn(bf, *P_shape, generator=gen) * 1e-3
        vf = O.project_onto_l1_ball(torch.rand(bf, k, generator=gen), 8 / 255)
        df = d.clone()
        sdf, svf, idx = O.AdamWState(df, 0.01), O.AdamWState(vf, 0.01), torch.arange(bf)
        t1 = time.perf_counter()
        O.synth(xf, df, vf[idx])
        O.apply_gradient_a(gf, idx, df, vf, sdf, svf, 8 / 255)
        dict_only_ms = (time.perf_counter() - t1) * 1e3
        del xf, gf
    out = {"value": value, "unit": "adversarial images/sec", "cores": threads, "kind": "port",
           "sample": f"{what}, fp32, torch {torch.__version__} CPU, {threads} threads of {os.cpu_count()} logical "
                     f"cores; configs[1] shape ({args.model}, {k} atoms, {P_shape[1]}x{P_shape[2]}) on {b} of its "
                     f"{args.batch} images per step; {dt:.1f} s"}
    if args.mode == "learn":
        out["label_policy"] = same
        out["value_recomputed_labels" if args.cache_labels else "value_cached_labels"] = other_value
        out["dictionary_ops_alone_ms_per_step"] = dict_only_ms
        out["dictionary_ops_alone_note"] = (f"synthesis + backward through the tensordot + AdamW(D, all rows of V) + l1 projection + clamp "
                                            f"on the host cores at the full batch of {args.batch} images, no classifier (one step)")
    if args.cpu_config1 and args.mode == "learn":
        out["config1"] = cpu_config1(dev)
    return out


TRANSFER_TARGETS = ("resnet18", "densenet121", "googlenet", "inception_v3", "mobilenet_v2", "vgg11")   # demo_dL_attack.py:41-53


class _SeededImages(torch.utils.data.Dataset):
    """n seeded U[0,1) images (3,S,S), generated item by item (nothing of size n*P is ever held on the host)."""

    def __init__(self, n, size, seed):
        self.n, self.size, self.seed = n, size, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return torch.rand(3, self.size, self.size, generator=torch.Generator().manual_seed(self.seed * 1_000_003 + i)), 0


def cpu_baseline_transfer(args, shape, b=4):
    """oracle.transfer_performance (performance.py:205-232 restated) on the host cores: b images of the bench workload,
    the same six target architectures (fp32, CPU), the attack = the oracle's forward_supervised_ddrague against the
    source architecture.  100 DDrague iterations on the CPU would take minutes, so the attack is timed at 1 and at 3
    iterations, which gives the per-iteration cost and the per-call fixed cost (labels, Gram / pseudo-inverse, final
    synthesis); the rate reported is b / (fixed + steps_inference * per_iteration + scoring) — stated in `sample`."""
    from oracle import adil_oracle as O
    from dl_attack_on_imagenet_amd import zoo
    threads = torch.get_num_threads()
    k, eps = args.atoms, 8 / 255
    g = torch.Generator().manual_seed(0)
    x = torch.rand(b, *shape, generator=g)
    d = -1 + 2 * torch.rand(*shape, k, generator=g)
    src = zoo.build_classifier(args.model, seed=0)
    targets = {name: zoo.build_classifier(name, seed=1 + i) for i, name in enumerate(TRANSFER_TARGETS)}
    O.forward_supervised_ddrague(src, x[:1], d, eps, 1, args.loss)                       # warm-up (allocators, MKL)
    t = {}
    for iters in (1, 3):
        t0 = time.perf_counter()
        adv = O.forward_supervised_ddrague(src, x, d, eps, iters, args.loss)
        t[iters] = time.perf_counter() - t0
    per_iter = (t[3] - t[1]) / 2
    fixed = max(t[1] - per_iter, 0.0)
    t0 = time.perf_counter()
    perf = O.transfer_performance(lambda xx, yy: adv, targets, [(x, torch.zeros(b, dtype=torch.long))], b)
    score = time.perf_counter() - t0
    full = fixed + args.steps_inference * per_iter + score
    return {"value": b / full, "unit": "attacked images/sec", "cores": threads, "kind": "port",
            "sample": f"oracle.transfer_performance on {b} of the bench's images, fp32, torch {torch.__version__} CPU, {threads} "
                      f"threads of {os.cpu_count()} logical cores: attack timed at 1 and 3 DDrague iterations ({t[1]:.1f} s, "
                      f"{t[3]:.1f} s -> {per_iter:.2f} s per iteration, {fixed:.2f} s fixed per call), scoring on the six "
                      f"targets {score:.1f} s; value = {b} / (fixed + {args.steps_inference} * per_iteration + scoring) = "
                      f"{b} / {full:.0f} s (extrapolated, not run in full)",
            "fooling_rates_of_the_3_iteration_adversary": {n: perf[n]["fooling_rate"] for n in perf}}


def bench_transfer(args, rank, world, dev, timer):
    """configs[3]: performance.get_transfer_performance (performance.py:183-232) over an evaluation set resident in HBM."""
    import tempfile
    import performance as perf
    from attacks import ADIL
    from dl_attack_on_imagenet_amd import dist as adist, loader, zoo
    sdtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    s_bytes = 2 if args.dtype == "bf16" else 4
    B, K, S = args.batch, args.atoms, args.image_size
    shape, P, eps = (3, S, S), 3 * S * S, 8 / 255
    fused = bool(args.fuse_bn_act) and zoo.canonical_name(args.model).startswith("resnet")
    source = zoo.build_classifier(args.model, seed=0, device=dev, dtype=sdtype, channels_last=bool(args.channels_last) and fused,
                                  fuse_bn_act=fused, fuse_stem=bool(args.fuse_stem and fused and args.dtype == "bf16"),
                                  head_fp32="inference" if (fused and args.dtype == "bf16") else False)
    targets = {name: zoo.build_classifier(name, seed=1 + i, device=dev, dtype=sdtype) for i, name in enumerate(TRANSFER_TARGETS)}
    tmp = tempfile.mkdtemp(prefix=f"adil_bench_rank{rank}_")
    gd0 = torch.Generator().manual_seed(7)                           # the same dictionary on every rank (one learned D, replicated)
    torch.save([-1 + 2 * torch.rand(*shape, K, generator=gd0), torch.zeros(1), [], [], torch.tensor(0.)],
               os.path.join(tmp, "ImageNet_bench.bin"))
    atk = ADIL(source, eps=eps, n_atoms=K, attack="supervised", model_name="bench", loss=args.loss, kappa=50,
               steps_inference=args.steps_inference, dict_dir=tmp, stream_dtype=sdtype)

    def loader_of(batches, seed):
        # performance.py hands batch i to rank i % world: a set of world * batches batches, of which this rank uploads
        # and keeps its own `batches` (weak scaling: every rank attacks `batches` batches of B images)
        n = world * batches * B
        return loader.ResidentBatches(_SeededImages(n, S, seed), torch.zeros(n, dtype=torch.long), B, dev, sdtype,
                                      shard=(rank, world))

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    warm = loader_of(max(args.warmup, 0), 1000) if args.warmup > 0 else None
    timed = loader_of(args.steps, 2000)
    if warm is not None:
        perf.get_transfer_performance({"adil": [atk]}, targets, warm, device=dev)
    sync()
    if timer is not None:
        timer.enabled = True
    t0 = time.perf_counter()
    result = perf.get_transfer_performance({"adil": [atk]}, targets, timed, device=dev)["adil"]
    sync()
    elapsed = time.perf_counter() - t0
    if timer is not None:
        timer.enabled = False
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {k: torch.tensor([result[n][k] for n in result], dtype=torch.float64)
                                         for k in ("fooling_rate", "rmse", "mse")})
    if world > 1:
        elapsed = float(adist.all_reduce_(torch.tensor([elapsed], dtype=torch.float64, device=dev), torch.distributed.ReduceOp.MAX))
    out = {
        "metric": "attacked images/sec (transfer evaluation: full attack(x, y) + six targets scored, classifiers included)",
        "value": world * B * args.steps / elapsed, "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": (f"performance.get_transfer_performance (BASELINE.json configs[3]): one learned-dictionary attack "
                                f"(ADiL forward_supervised_DDrague, {args.steps_inference} iterations with the stop test, {K} atoms, "
                                f"loss={args.loss}) against {args.model}, adversary scored on {len(targets)} targets "
                                f"({', '.join(targets)}), {B} images per batch, {args.steps} batches per GPU, {S}x{S}, {args.dtype} "
                                f"image streams, fp32 z + AdamW moments; evaluation set resident in HBM (loader.ResidentBatches)"),
                   "classifier": f"random-init {args.model} (source{', FusedResNet with fp32 logits inside the DDrague loop (head_fp32=inference)' if fused else ''}) and six random-init targets, frozen, eval",
                   "global_batch": world * B, "atoms": K, "steps_inference": args.steps_inference,
                   "parallelism": f"dp{world}: batches dealt to ranks (performance.py path), D replicated, final sums all-reduced",
                   "collective": {"backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None,
                                  "world_size": world, adist.IPC_ENV: os.environ.get(adist.IPC_ENV)},
                   "transfer_fooling_rates": {n: result[n]["fooling_rate"] for n in result},
                   "rmse": next(iter(result.values()))["rmse"]},
    }
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)                        # the synthetic dictionary file (60 MB at 100 atoms)
    if not args.full:
        return out
    kern_ms = timer.summary_ms()
    launches = {k: len(v) for k, v in timer.records.items()}
    alg = algorithmic_bytes(B, P, K, B, s_bytes, "inference")
    dom = max((k for k in kern_ms if k in alg), key=lambda k: kern_ms[k] * launches[k])
    achieved = alg[dom] / (kern_ms[dom] * 1e-3) / 1e9
    out["config"]["ddrague_iterations_run_per_batch"] = (launches.get("zstep_", 0) + launches.get("zstep_codes_", 0)) / max(args.steps, 1)
    out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": achieved / HBM_PEAK_GBS, "traffic": measured_traffic(dom, K),
                       "mfma_utilisation": measured_mfma_utilisation(dom, K),
                       "algorithmic_bytes_per_launch": alg[dom], "avg_launch_ms": kern_ms[dom], "launches_timed": launches[dom],
                       "empty_event_bracket_ms": timer.empty_bracket_ms()}
    out["kernels_ms_per_launch"], out["kernel_launches_timed"] = kern_ms, launches
    out["dictionary_path_ms_per_step"] = sum(kern_ms[k] * launches[k] for k in kern_ms) / args.steps
    if rank == 0 and world == 1 and args.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_transfer(args, shape)
    return out


def measured_traffic(group, atoms):
    """HBM bytes per launch of a launch group from the PMC passes (profiles/hbm_traffic.json, written by tools/pmc_traffic.py
    from two separate rocprofv3 --pmc runs): only when the file was collected from THIS build of the kernels (it records
    the hash of csrc/ + include/ it was measured on) and at this atom count; otherwise null."""
    tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json" if atoms == 50 else f"hbm_traffic_k{atoms}.json")
    try:
        from dl_attack_on_imagenet_amd.build import source_hash
        rec = json.load(open(tpath))
        if rec.get("_source", {}).get("kernel_source_hash") != source_hash() or rec.get("_source", {}).get("atoms", 50) != atoms:
            return None
        return rec.get(group)
    except Exception:
        return None


def measured_mfma_utilisation(group, atoms):
    """Share of the matrix pipes' cycles the group's kernel keeps busy, from the PMC pass of tools/run_profiles.sh mfma
    (profiles/mfma_utilisation*.json: SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8)); like the traffic, only
    when the file was collected from THIS build of the kernels at this atom count, otherwise null.  Supporting evidence:
    the bound of every kernel on the path is HBM."""
    mpath = os.path.join(ROOT, "profiles", "mfma_utilisation.json" if atoms == 50 else f"mfma_utilisation_k{atoms}.json")
    try:
        from dl_attack_on_imagenet_amd.build import source_hash
        rec = json.load(open(mpath))
        if rec.get("_source", {}).get("kernel_source_hash") != source_hash() or rec.get("_source", {}).get("atoms", 50) != atoms:
            return None
        return rec.get(group)
    except Exception:
        return None


def spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no torchrun environment: start the N ranks ourselves.  This parent has
    made no GPU call (importing torch does not initialise HIP) and never will: the ranks are fresh child processes
    of `python -m torch.distributed.run`, one per GPU, rendezvous on 127.0.0.1; rank 0 prints the JSON line, which
    passes through on the inherited stdout; the parent exits with the launcher's return code."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)         # HSA_ENABLE_IPC_MODE_LEGACY: also set by dist.init_from_env inside every rank, whoever launched it
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(1, args.gpus))))
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args))
    from dl_attack_on_imagenet_amd import dist as adist
    rank, world, local_rank = adist.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the ADiL hot path has no CPU fallback")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}; launch N>1 with torch.distributed.run")
    dev = torch.device("cuda", adist.local_device_index(local_rank))
    torch.cuda.set_device(dev)

    from dl_attack_on_imagenet_amd import engine, ops, zoo
    timer = KernelTimer(ops) if args.full else None
    if args.mode == "transfer":
        out = bench_transfer(args, rank, world, dev, timer)
        if rank == 0:
            print(json.dumps(out), flush=True)
        if torch.distributed.is_initialized():
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        return
    sdtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    s_bytes = 2 if args.dtype == "bf16" else 4
    B, K, S = args.batch, args.atoms, args.image_size
    shape = (3, S, S)
    P = 3 * S * S
    eps = 8 / 255

    model = zoo.build_classifier(args.model, seed=0, device=dev, dtype=sdtype, channels_last=bool(args.channels_last),
                                 fold_bn=bool(args.fold_bn), pad_input_channels=args.pad_cin,
                                 fuse_bn_act=bool(args.fuse_bn_act),
                                 fuse_stem=bool(args.fuse_stem and args.fuse_bn_act and args.dtype == "bf16"
                                                and zoo.canonical_name(args.model).startswith("resnet")),
                                 # the bf16 FusedResNet's logits in fp32 INSIDE the DDrague inference loop only (engine.precise_head;
                                 # the learner keeps the bf16 head): +1.5 ... 2.5 pp ASR at no cost, profiles/r04_asr_gap.md
                                 head_fp32="inference" if (args.fuse_bn_act and args.dtype == "bf16"
                                                           and zoo.canonical_name(args.model).startswith("resnet")) else False)
    gen = torch.Generator().manual_seed(1000 + rank)                 # each rank owns different images (weak scaling)
    x = torch.rand(B, *shape, generator=gen).to(dev).to(sdtype).contiguous()
    gd0 = torch.Generator().manual_seed(7)                           # the same D0 on every rank
    d = (-1 + 2 * torch.rand(*shape, K, generator=gd0)).to(dev)
    v = ops.l1ball_project_(torch.rand(B, K, generator=gen).to(dev), eps)
    # ADIL_FORCE_REDUCER=1 exercises the RCCL path (process group, all-reduce of grad_d) even with one rank
    force = os.environ.get("ADIL_FORCE_REDUCER") == "1" and torch.distributed.is_initialized()
    reducer = adist.DictGradReducer(timing=args.full) if (world > 1 or force) else None
    if args.mode == "inference":
        solver = engine.DDragueSolver(model, x, d, eps, args.loss, False, 50.0)          # Gram / pseudo-inverse: once per call

        def step():
            solver.iterate()                                  # no host sync: the stop test is left to the caller
            return None, None
    else:
        learner = engine.DictionaryLearner(d, v, eps, 0.01, args.loss, False, 50.0, reducer=reducer,
                                           fp8_synth=bool(args.fp8_synth))
        index = torch.arange(B, device=dev)
        rows = list(range(B))
        cache = engine.LabelCache(B, dev) if args.cache_labels else None      # labels on the first visit, as the learners do

        def step():
            return learner.step(model, x, index, cache.get(model, x, index, rows) if cache is not None else None)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    if reducer is not None:                                   # communicator set-up is not a step (matters with --warmup 0)
        reducer.all_reduce_(torch.zeros(1, device=dev))
    for _ in range(args.warmup):
        step()
    sync()
    if reducer is not None:
        reducer.reset_timing()                                # brackets of the timed steps only
    if timer is not None:
        timer.enabled = True
    t0 = time.perf_counter()
    loss, fooled = None, None
    for _ in range(args.steps):
        loss, fooled = step()
    sync()
    elapsed = time.perf_counter() - t0
    if timer is not None:
        timer.enabled = False
    if args.mode == "inference":
        adv, codes = solver.result()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(adversarial_images=adv, codes=codes) if args.mode == "inference" else
                     dict(d=learner.d, v=learner.v, loss=loss, fooled=fooled))
    # what the collective cost: backend, world size, mean start -> wait bracket of the step's all-reduce (HIP events on
    # the compute stream; contains the code-row update that runs underneath); a 1-rank run has no collective
    collective = reducer.describe() if reducer is not None else {
        "backend": None, "world_size": world, "bytes_per_allreduce": 0,
        adist.IPC_ENV: os.environ.get(adist.IPC_ENV)}
    if reducer is not None:
        reducer.timing = False
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        elapsed = float(adist.all_reduce_(tmax, torch.distributed.ReduceOp.MAX))
    other_variant = None
    if args.mode == "learn" and args.full:
        # informational, never `value`: the same steps with the OTHER pseudo-label policy — recomputed in every step (the
        # reference's 2 forwards + 1 backward) when the headline caches them, cached when it recomputes
        fixed = None if args.cache_labels else engine.predict(model, x)
        sync()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            learner.step(model, x, index, fixed)
        sync()
        e2 = time.perf_counter() - t1
        if world > 1:
            e2 = float(adist.all_reduce_(torch.tensor([e2], dtype=torch.float64, device=dev), torch.distributed.ReduceOp.MAX))
        other_variant = {"images_per_sec": world * B * args.steps / e2, "ms_per_step": e2 / args.steps * 1e3,
                         "note": ("pseudo-labels recomputed in every step: the reference's op sequence, 2 fwd + 1 bwd (--cache-labels 0)"
                                  if args.cache_labels else "pseudo-labels cached per image, 1 fwd + 1 bwd per step (--cache-labels 1)")}

    if args.mode == "inference":
        fool_rate = float((engine.predict(model, adv) != solver.labels).float().mean())
    else:
        fool_rate = float(fooled) / B
    out = {
        "metric": "adversarial images/sec (ADiL learning step, classifier included)" if args.mode == "learn" else
                  "adversarial images/sec (ADiL DDrague inference iteration, classifier included)",
        "value": world * B * args.steps / elapsed,
        "unit": "images/sec",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": (f"ADiL learn_dictionary_a step vs {args.model}, {B} images/GPU, {K} atoms, "
                                f"{S}x{S}, {args.dtype} image streams + fp32 D/V master"
                                f"{', fp8 (e4m3) operands in the synthesis contraction, read from the persistent fp8 copy of D that the AdamW launch maintains [measured: no faster than bf16 operands — 86.1 vs 85.8 us per synthesis at 100 atoms, +2.5 us in AdamW(D): the synthesis is bound by its 2 B P s image streams and by occupancy, not by the 45 MB of dictionary the copy saves; a precision variant, not a speed-up]' if args.fp8_synth else ''}, loss={args.loss}, "
                                + ("clean pseudo-labels computed once per image and cached (1 fwd + 1 bwd per step; result-neutral, "
                                   "profiles/r03_label_stability.md)" if args.cache_labels else
                                   "clean pseudo-labels recomputed in every step (the reference's op sequence, 2 fwd + 1 bwd)"))
                   if args.mode == "learn" else
                   (f"ADiL forward_supervised_DDrague iteration (the attack(x, y) path of transfer evaluation) vs "
                    f"{args.model}, {B} images/GPU, {K} atoms, {S}x{S}, {args.dtype} image streams, fp32 z + AdamW "
                    f"moments, loss={args.loss}, clean labels computed once (constant; 1 fwd + 1 bwd per iteration)"),
                   "classifier": f"random-init {args.model}, frozen, eval; channels_last={args.channels_last}, "
                                 f"bn_act_epilogue_fused={args.fuse_bn_act}, bn_folded={args.fold_bn}, "
                                 f"first_conv_cin_padded_to={args.pad_cin} (unused with stem kernels), stem_kernels={args.fuse_stem}, "
                                 f"pointwise_convs=fused GEMM+epilogue kernels (fwd and input gradient), "
                                 f"stride1_3x3_convs=adil_conv3x3, head=bf16 while learning / fp32 logits inside the DDrague "
                                 f"inference loop (zoo head_fp32='inference')",
                   "global_batch": world * B, "atoms": K, "inner_iters": args.steps,
                   "parallelism": f"dp{world}: images+codes sharded, D replicated, 1 all-reduce(grad_d)/step",
                   "collective": collective,
                   ("train_fooling_rate_last_step" if args.mode == "learn" else "fooling_rate_after_timed_iterations"): fool_rate},
    }
    if args.full:
        kern_ms = timer.summary_ms()
        alg = algorithmic_bytes(B, P, K, B, s_bytes, args.mode)
        dom = max((k for k in kern_ms if k in alg), key=lambda k: kern_ms[k])
        achieved = alg[dom] / (kern_ms[dom] * 1e-3) / 1e9
        traffic = measured_traffic(dom, K)                          # from separate rocprofv3 --pmc runs of THIS build, else null
        # per step, not per launch: a DDrague iteration launches pack_codes twice (the codes of the z-step, the code gradient)
        launches = {k: len(v) for k, v in timer.records.items()}
        per_step = {k: launches.get(k, 0) / max(args.steps, 1) for k in kern_ms}
        dict_ms = sum(kern_ms[k] * per_step[k] for k in kern_ms)
        out["roofline"] = {
            "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
            "mfma_utilisation": measured_mfma_utilisation(dom, K),     # PMC pass of this build, else null
            "algorithmic_bytes_per_launch": alg[dom], "avg_launch_ms": kern_ms[dom],
            "empty_event_bracket_ms": timer.empty_bracket_ms(),
            # informational: what a cold read + write stream of the synth's image bytes reaches on this pool, whatever its
            # access pattern — a flat grid-stride copy included (tools/exp/stream_patterns.hip, profiles/r04_stream_patterns.md)
            "measured_copy_ceiling_GBps": 5100.0,
            # informational: the same with the cost of an empty event bracket taken off (this is the figure that
            # agrees with rocprofv3's kernel duration to ~1 %, profiles/README.md); `achieved`/`frac` stay raw
            "frac_minus_empty_bracket": alg[dom] / (max(kern_ms[dom] - timer.empty_bracket_ms(), 1e-6) * 1e-3) / 1e9
                                        / HBM_PEAK_GBS}
        out["kernels_ms_per_step"] = kern_ms
        out["dictionary_path_ms_per_step"] = dict_ms
        out["dictionary_path_algorithmic_GBps"] = sum(alg[k] * per_step[k] for k in kern_ms if k in alg) / (dict_ms * 1e-3) / 1e9
        out["kernel_launches_per_step"] = per_step
    if other_variant is not None:
        out["config"]["recomputed_labels_variant" if args.cache_labels else "cached_labels_variant"] = other_variant
        # both pseudo-label policies at the top level as well, so that neither number has to be dug out of `config`:
        # `value` follows --cache-labels (default 1); the reference's 2 fwd + 1 bwd sequence is always here
        out["value_reference_op_sequence_recomputed_labels"] = (other_variant if args.cache_labels else
                                                                {"images_per_sec": out["value"], "ms_per_step": out["ms_per_step"]})["images_per_sec"]
        out["value_cached_labels"] = out["value"] if args.cache_labels else other_variant["images_per_sec"]
        # `value` changed definition between BENCH_r02 (recomputed labels, 2 fwd + 1 bwd) and BENCH_r03 onwards
        # (cached labels, 1 fwd + 1 bwd).  Round-over-round tracking compares `value_reference_op_sequence_recomputed_labels`
        # with r02's `value`; `cpu_baseline.value` follows the policy of `value` and carries the other policy next to it.
        out["value_definition"] = (
            ("clean pseudo-labels cached per image (1 classifier forward + 1 backward per step; the learners' default since "
             "round 3, result-neutral: SURVEY.md section 8(d), quirk Q4, profiles/r03_label_stability.md)" if args.cache_labels else
             "clean pseudo-labels recomputed in every step (the reference's op sequence, 2 forwards + 1 backward)")
            + "; BENCH_r02.value used the recomputing sequence: compare it with value_reference_op_sequence_recomputed_labels. "
              "The bench replays one resident batch, so the cache always hits — as it does from an image's second epoch on in a "
              "run of the learner (500 epochs in demo_dL_attack.py:92); the first epoch pays the reference's sequence.")
    if rank == 0 and world == 1 and args.full and args.cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, shape, dev)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if torch.distributed.is_initialized():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
