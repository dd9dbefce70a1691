"""Child process of tests/test_gpu_attention.py::test_attention_is_bitwise_across_processes: runs adil_attn_fwd and
adil_attn_bwd (through ops.attention and autograd) on seeded gaussian operands of three shapes and prints one sha256 per
output."""
import hashlib
import sys

import torch

import attention_reference as aref

# (B, T, H)
SHAPES = [(2, 197, 12), (3, 33, 2), (1, aref.MAX_TOKENS, 3)]


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import ops
    dev = torch.device("cuda", 0)
    for i, (b, t, h) in enumerate(SHAPES):
        op = aref.operands("child/%d" % i, "gaussian", b, t, h)
        qkv = op.qkv.to(dev).requires_grad_(True)
        o = ops.attention(qkv, h)
        (g,) = torch.autograd.grad(o, qkv, op.go.to(dev))
        print("hash o%d %s" % (i, digest(o)), flush=True)
        print("hash gqkv%d %s" % (i, digest(g)), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
