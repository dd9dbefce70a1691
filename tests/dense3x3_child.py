"""Child process of tests/test_gpu_dense3x3.py::test_dense3x3_is_bitwise_across_processes: runs adil_dense3x3_fwd and
adil_dense3x3_bwd (through ops.dense3x3_conv and autograd) on seeded gaussian operands of three rows and prints one sha256
per output."""
import hashlib
import sys

import torch

import dense3x3_reference as dref


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, c, n) in enumerate(dref.HASH_ROWS):
        op = dref.operands("child/%d" % i, "gaussian", b, h, w, c, n)
        wf, wb = (t.to(dev) for t in ops.pack_conv3x3_weights(op.w))
        x = op.x.to(dev).permute(0, 3, 1, 2).requires_grad_(True)
        y = ops.dense3x3_conv(x, wf, wb)
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash gx%d %s" % (i, digest(gx.permute(0, 2, 3, 1))), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
