"""The configs[1] learning step (ResNet-50, 512 images, 50 atoms, bf16 image streams, cached labels) on the two resident
stores, timed in ONE process, alternating: the bf16 store (ResidentImages(dtype=bfloat16): gather the batch, then
synthesize from the copy) and the 8-bit store (ResidentImages(dtype=uint8): synthesize straight from the bytes,
ops.synth_store).  Prints one JSON line: resident bytes of both stores, per-step times of both, and the bytes per step
of the data step + synthesis computed from the shapes.

usage: python tools/bench_image_store.py [--images 2048] [--rounds 6] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dl_attack_on_imagenet_amd import engine, ops, zoo  # noqa: E402
from dl_attack_on_imagenet_amd.build import source_hash  # noqa: E402
from dl_attack_on_imagenet_amd.loader import ResidentImages  # noqa: E402


class _Images(torch.utils.data.Dataset):
    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=2048, help="resident images (the step draws 512 of them)")
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--atoms", type=int, default=50)
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=10, help="steps per store per round")
    p.add_argument("--warmup", type=int, default=3)
    args = p.parse_args()
    dev = torch.device("cuda", 0)
    n, b, k, eps = args.images, args.batch, args.atoms, 8 / 255
    shape = (3, 224, 224)
    pix = 3 * 224 * 224
    u8 = torch.randint(0, 256, (n,) + shape, generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    stores = {"bf16": ResidentImages(_Images(u8.float().div(255)), dev, torch.bfloat16),
              "uint8": ResidentImages(_Images(u8), dev, torch.uint8, stream_dtype=torch.bfloat16)}
    del u8
    model = zoo.build_classifier("resnet50", seed=0, device=dev, dtype=torch.bfloat16, channels_last=True, fold_bn=True,
                                 pad_input_channels=8, fuse_bn_act=True, fuse_stem=True, head_fp32="inference")
    g = torch.Generator().manual_seed(7)
    d0 = -1 + 2 * torch.rand(*shape, k, generator=g)
    v0 = torch.rand(n, k, generator=g)
    learners = {name: engine.DictionaryLearner(d0.to(dev), ops.l1ball_project_(v0.to(dev), eps), eps, 0.01, "logits", False,
                                               50.0) for name in stores}
    caches = {name: engine.LabelCache(n, dev) for name in stores}
    order = [list(range(i, i + b)) for i in range(0, n - b + 1, b)]
    at = {name: 0 for name in stores}

    def step(name):
        store, learner, cache = stores[name], learners[name], caches[name]
        rows = order[at[name] % len(order)]
        at[name] += 1
        index = store.index_tensor(rows)
        if name == "bf16":                                        # the learner's data step today: gather, then synthesize
            x = store.gather(index)
            return learner.step(model, x, index, cache.get(model, x, index, rows))
        return learner.step(model, store, index, cache.get(model, lambda: store.gather(index), index, rows))

    for name in stores:                                           # labels of every image cached, libraries tuned
        for _ in range(max(args.warmup, len(order))):
            step(name)
    torch.cuda.synchronize()
    times = {name: [] for name in stores}
    for _ in range(args.rounds):
        for name in stores:
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    s = 2                                                         # bytes per stream element (bf16)
    traffic = {
        # gather: read B P s of the store, write B P s; synth: read x (B P s) + D (P K 4), write x + D v (B P s)
        "bf16": {"gather": 2 * b * pix * s, "synth": 2 * b * pix * s + pix * k * 4},
        # synth_store: read B P bytes through the index + D, write B P s; no gather
        "uint8": {"gather": 0, "synth": b * pix * 1 + pix * k * 4 + b * pix * s},
    }
    out = {
        "what": "configs[1] learning step (resnet50 bf16, 512 images, 50 atoms, cached labels), bf16 store vs 8-bit store, "
                "alternating rounds in one process",
        "source_hash": source_hash(),
        "device": torch.cuda.get_device_name(dev),
        "resident_images": n,
        "resident_bytes": {name: st.images.numel() * st.images.element_size() for name, st in stores.items()},
        "ms_per_step": {name: {"median": sorted(t)[len(t) // 2], "min": min(t), "rounds": [round(x, 3) for x in t]}
                        for name, t in times.items()},
        "bytes_per_step_data_and_synth": {name: dict(v, total=sum(v.values())) for name, v in traffic.items()},
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
