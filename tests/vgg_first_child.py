"""Child process of tests/test_gpu_vgg_first.py::test_first_group_is_bitwise_across_processes: runs the VGG first-group
kernels (through ops.first_conv3x3_pool and autograd) on seeded gaussian operands of three rows and prints one sha256 each
for y, idx and gx."""
import hashlib
import sys

import torch

import vgg_first_reference as vf


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, h, w, dtype) in enumerate(vf.HASH_ROWS):
        op = vf.operands("child/%d" % i, "gaussian", b, h, w, dtype)
        wf, wb = (t.to(dev) for t in ops.pack_first3x3_pool_weights(op.w))
        x = op.x.to(dev).requires_grad_(True)
        y = ops.first_conv3x3_pool(x, wf, wb, op.bias.to(dev), op.mean, op.inv_std)
        (idx,) = [t for t in y.grad_fn.saved_tensors if t.dtype == torch.uint8]
        (gx,) = torch.autograd.grad(y, x, op.g.to(dev).permute(0, 3, 1, 2))
        print("hash y%d %s" % (i, digest(y.permute(0, 2, 3, 1))), flush=True)
        print("hash idx%d %s" % (i, digest(idx)), flush=True)
        print("hash gx%d %s" % (i, digest(gx)), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
