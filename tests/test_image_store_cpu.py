"""CPU: the 8-bit image store option — ADIL's `image_store` argument, the refusals of the store and of its kernels on
CPU tensors (no fallback), and the new ctypes signatures."""
import ctypes

import pytest
import torch


class _Images(torch.utils.data.Dataset):
    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], 0


def test_adil_image_store_option():
    from attacks import ADIL
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(12, 3))
    assert ADIL(net, eps=0.1).image_store is None                      # default: the stream-dtype store
    assert ADIL(net, eps=0.1, image_store=None).image_store is None
    assert ADIL(net, eps=0.1, image_store="uint8").image_store == "uint8"
    for bad in ("bf16", "u8", torch.uint8, 8, ""):
        with pytest.raises(ValueError, match="image_store"):
            ADIL(net, eps=0.1, image_store=bad)


def test_byte_store_refuses_cpu():
    from dl_attack_on_imagenet_amd import ops
    from dl_attack_on_imagenet_amd.loader import ResidentBatches, ResidentImages
    ds = _Images(torch.zeros(4, 3, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ResidentImages(ds, "cpu", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ResidentBatches(ds, torch.zeros(4, dtype=torch.int64), 2, "cpu", dtype=torch.uint8, stream_dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.images_to_u8(torch.zeros(8), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_images(torch.zeros(2, 8, dtype=torch.uint8), None, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.synth_store(torch.zeros(2, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(8, 1),
                        torch.zeros(32, 16), 1, torch.float32)


def test_store_signatures_load():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    lib = _lib.load()
    assert _lib.ABI_VERSION == 8 and lib.adil_abi_version() == 8
    assert lib.adil_max_atoms() == 128
    for name, nargs in (("adil_images_to_u8", 6), ("adil_synth_store", 12)):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    # argument checks run on the host, before any launch: null pointers / bad sizes / unsupported dtypes are refused
    assert lib.adil_images_to_u8(None, 0, None, 8, None, None) == -1
    assert lib.adil_synth_store(None, None, None, None, None, 1, 8, 1, 0, -1.0, 0, None) == -1
    assert lib.adil_gather_images(None, 2, None, None, 0, 1, 8, None) == -1
