"""Child process of tests/test_gpu_pointwise8.py::test_pw8_is_bitwise_across_processes: runs adil_pw8_fwd and adil_pw8_bwd
(through ops.pw8_conv and autograd) on seeded gaussian operands of three rows and prints one sha256 per output."""
import hashlib
import sys

import torch

import pointwise8_reference as pref

# (B, H, W, K, N, act, res)
SHAPES = [(8, 28, 28, 32, 192, 1, False), (8, 14, 14, 576, 96, 0, True), (3, 7, 5, 24, 40, 0, False)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, k, n, act, with_res) in enumerate(SHAPES):
        op = pref.operands("child/%d" % i, "gaussian", b * h * w, k, n, with_res)
        nchw = lambda t: t.to(dev).reshape(b, h, w, -1).permute(0, 3, 1, 2)
        x = nchw(op.x).requires_grad_(True)
        y = ops.pw8_conv(x, op.w.to(dev), op.wt.to(dev), op.scale.to(dev), op.shift.to(dev), nchw(op.res) if with_res else None,
                         bool(act))
        (gx,) = torch.autograd.grad(y, x, nchw(op.g))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
