"""Child process of tests/test_gpu_dense_head.py::test_dense_head_is_bitwise_across_processes: prints one sha256 each of the
logits and of the input gradient of the six-switch DenseNet-121 (`own_dense_head=True` on top of the five dense switches) on 4
seeded images at 64 x 64.  The parent computes the same two digests in its own process with `network_digests`."""
import hashlib
import sys

import torch

SIX = dict(own_dense_pointwise=True, own_dense_conv=True, own_dense_block=True, own_dense_transition=True, own_dense_stem=True,
           own_dense_head=True)


def digest(t):
    t = t.detach().contiguous()
    h = hashlib.sha256()
    h.update(str((tuple(t.shape), str(t.dtype))).encode())
    h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def network_digests():
    from dl_attack_on_imagenet_amd import zoo
    dev = torch.device("cuda", 0)
    model = zoo.build_classifier("densenet121", num_classes=10, seed=3, device=dev, dtype=torch.bfloat16, channels_last=True, **SIX)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(21)).to(dev).bfloat16().requires_grad_(True)
    logits = model(x)
    assert logits.dtype == torch.float32
    (gx,) = torch.autograd.grad(logits.square().sum(), x)
    torch.cuda.synchronize()
    return ["hash net_logits %s" % digest(logits), "hash net_gx %s" % digest(gx)]


if __name__ == "__main__":
    for line in network_digests():
        print(line, flush=True)
    sys.exit(0)
