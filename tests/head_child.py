"""Child process of tests/test_gpu_head.py::test_head_is_bitwise_across_processes: runs adil_pool_head_fwd and
adil_pool_head_bwd through the C ABI on seeded gaussian operands of three rows and prints one sha256 per output (pooled,
logits, gpooled, gx), then the logits and the input gradient of the all-switches MobileNetV2 with the fp32 head on 8 seeded
images at 64 x 64."""
import hashlib
import sys

import torch

import head_reference as href

# (B, HW, C, N)
SHAPES = [(8, 49, 1280, 1000), (3, 49, 24, 10), (17, 9, 40, 7)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import _lib, ops, zoo
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    for i, (b, hw, c, n) in enumerate(SHAPES):
        op = href.operands("child/%d" % i, "gaussian", b, hw, c, n)
        x, w, bias, g = (t.to(dev) for t in (op.x, op.w, op.bias, op.g))
        wt = w.t().contiguous()
        pooled, gpooled = torch.empty(b, c, device=dev), torch.empty(b, c, device=dev)
        logits, gx = torch.empty(b, n, device=dev), torch.empty(b, hw, c, dtype=torch.bfloat16, device=dev)
        rc = lib.adil_pool_head_fwd(ops._ptr(x), ops._ptr(wt), ops._ptr(bias), ops._ptr(pooled), ops._ptr(logits), b, hw, c, n,
                                    ops._stream())
        rc = rc or lib.adil_pool_head_bwd(ops._ptr(g), ops._ptr(w), ops._ptr(gpooled), ops._ptr(gx), b, hw, c, n, ops._stream())
        if rc != 0:
            print("rc", rc)
            return 1
        for name, t in (("pooled", pooled), ("logits", logits), ("gpooled", gpooled), ("gx", gx)):
            print("hash %s%d %s" % (name, i, digest(t)), flush=True)
    model = zoo.build_classifier("mobilenet", num_classes=10, seed=3, device=dev, dtype=torch.bfloat16, channels_last=True,
                                 own_depthwise=True, own_pointwise=True, own_first_conv=True, head_fp32=True)
    x = torch.rand(8, 3, 64, 64, generator=torch.Generator().manual_seed(21)).to(dev).bfloat16().requires_grad_(True)
    logits = model(x)
    (gx,) = torch.autograd.grad(logits.square().sum(), x)
    print("hash net_logits %s" % digest(logits), flush=True)
    print("hash net_gx %s" % digest(gx), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
