"""Child process of tests/test_gpu_dense1x1.py::test_dense1x1_is_bitwise_across_processes: runs adil_dense1x1_fwd and
adil_dense1x1_bwd (through ops.dense1x1_conv and autograd) on seeded gaussian operands of three rows and prints one sha256
per output."""
import hashlib
import sys

import torch

import dense1x1_reference as dref

# (B, H, W, K, N, act)
SHAPES = [(4, 14, 14, 416, 128, 1), (4, 7, 7, 512, 256, 0), (3, 7, 5, 24, 40, 1)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, k, n, act) in enumerate(SHAPES):
        op = dref.operands("child/%d" % i, "gaussian", b * h * w, k, n)
        nchw = lambda t: t.to(dev).reshape(b, h, w, -1).permute(0, 3, 1, 2)
        x = nchw(op.x).requires_grad_(True)
        y = ops.dense1x1_conv(x, op.pscale.to(dev), op.pshift.to(dev), op.w.to(dev), op.wt.to(dev), op.scale.to(dev),
                              op.shift.to(dev), bool(act))
        (gx,) = torch.autograd.grad(y, x, nchw(op.g))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
