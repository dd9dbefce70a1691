"""Child process of tests/test_gpu_vgg_conv.py::test_vgg_kernels_are_bitwise_across_processes: runs adil_conv3x3_wide
(through ops.conv3x3_wide and autograd) on seeded gaussian operands of three rows and the bias + ReLU + pool pair (through
ops.bias_relu_pool2 and autograd) on two, and prints one sha256 per output."""
import hashlib
import sys

import torch

import vgg_conv_reference as vref


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, c, n) in enumerate(vref.HASH_ROWS):
        op = vref.operands("child/%d" % i, "gaussian", b, h, w, c, n)
        wf, wb = (t.to(dev) for t in ops.pack_conv3x3_weights(op.w))
        x = op.x.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.conv3x3_wide(x, wf, wb)
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    for i, (b, h, w, c) in enumerate(vref.POOL_HASH_ROWS):
        op = vref.pool_operands("child/pool/%d" % i, "gaussian", b, h, w, c, True)
        x = op.x.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.bias_relu_pool2(x, op.bias.to(dev))
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash py%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash pgx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
