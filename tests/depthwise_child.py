"""Child process of tests/test_gpu_depthwise.py::test_dw3x3_is_bitwise_across_processes: runs adil_dw3x3_fwd and
adil_dw3x3_bwd (through ops.dw_conv3x3 and autograd) on seeded gaussian operands of three shapes and prints one sha256 per
output."""
import hashlib
import sys

import torch

import depthwise_reference as dref

SHAPES = [(8, 56, 56, 144, 2, 1), (8, 14, 14, 576, 1, 1), (4, 15, 13, 24, 2, 0)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, c, s, relu6) in enumerate(SHAPES):
        op = dref.operands("child/%d" % i, "gaussian", b, h, w, c, s)
        x = op.x.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.dw_conv3x3(x, op.w9c.to(dev), op.bias.to(dev), s, bool(relu6))
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
