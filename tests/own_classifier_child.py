"""Child process of tests/test_gpu_conv_s2.py::test_own_classifier_is_bitwise_across_processes: builds the ResNet-50 that
runs on this repository's kernels only (fuse_bn_act + fuse_stem + own_strided_conv) from a seed, runs forward + input
gradient on a seeded batch and prints one sha256 per block output, of the logits and of the input gradient."""
import hashlib
import sys

import torch


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        t = t.detach().contiguous()
        h.update(str((tuple(t.shape), str(t.dtype))).encode())
        h.update(t.view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()[:32]


def main():
    from dl_attack_on_imagenet_amd import zoo
    dev = torch.device("cuda", 0)
    model = zoo.build_classifier("resnet50", num_classes=1000, seed=11, device=dev, dtype=torch.bfloat16, channels_last=True,
                                 fuse_bn_act=True, fuse_stem=True, own_strided_conv=True)
    net = model[0]
    hooks = []
    for i, blk in enumerate(net.layers):
        def hook(mod, args, out, i=i):
            ts = [t for t in (out if isinstance(out, tuple) else (out,)) if isinstance(t, torch.Tensor)]
            print("hash block%02d %s" % (i, digest(*ts)), flush=True)
        hooks.append(blk.register_forward_hook(hook))
    x = torch.rand(32, 3, 224, 224, generator=torch.Generator().manual_seed(7)).to(dev).bfloat16().requires_grad_(True)
    logits = model(x)
    print("hash logits %s" % digest(logits), flush=True)
    (g,) = torch.autograd.grad(logits.float().square().sum(), x)
    print("hash input_gradient %s" % digest(g), flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
