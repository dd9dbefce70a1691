"""Child process of tests/test_gpu_first_conv.py::test_first_conv_is_bitwise_across_processes: runs adil_first3x3_fwd and
adil_first3x3_bwd (through ops.first_conv3x3 and autograd) on seeded gaussian operands of three rows and prints one sha256
per output."""
import hashlib
import sys

import torch

import first_conv_reference as fref

# (B, H, W, x dtype)
SHAPES = [(4, 64, 64, torch.bfloat16), (2, 33, 35, torch.float32), (3, 7, 9, torch.bfloat16)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, dtype) in enumerate(SHAPES):
        op = fref.operands("child/%d" % i, "gaussian", b, h, w, dtype)
        wf, wb = ops.pack_first3x3_weights(op.w.to(dev))
        x = op.x.to(dev).requires_grad_(True)
        y = ops.first_conv3x3(x, wf, wb, op.scale.to(dev), op.shift.to(dev), op.mean, op.inv_std, True)
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx)), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
