"""CPU: host side of the stem backward's kernel switch (adil_stem_bwd_variant): the built library exports the symbol, the
header declares it and _lib.py binds it under ABI 8; the switch keeps the contract of adil_conv3x3_loop; the two product
entry points keep their arguments and refuse what they refused under either value."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    return _lib, _lib.load()


def test_library_exports_header_declares_and_lib_binds_the_switch():
    _lib, bound = _bound()
    raw = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert hasattr(raw, "adil_stem_bwd_variant")
    assert re.search(r"\bint\s+adil_stem_bwd_variant\s*\(\s*int\s+\w+\s*\)\s*;", code)
    restype, argtypes = _lib.SIGNATURES["adil_stem_bwd_variant"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_int]
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # the product calls stay as they were
    assert len(_lib.SIGNATURES["adil_stem_pool_bwd"][1]) == 10
    assert len(_lib.SIGNATURES["adil_stem_conv_bwd"][1]) == 11


def test_switch_returns_the_previous_value_and_ignores_other_arguments():
    _, lib = _bound()
    first = lib.adil_stem_bwd_variant(1)
    try:
        assert lib.adil_stem_bwd_variant(0) == 1
        assert lib.adil_stem_bwd_variant(1) == 0
        for other in (2, -1, 7, 1 << 30):
            assert lib.adil_stem_bwd_variant(other) == 1         # a query: nothing changes
        assert lib.adil_stem_bwd_variant(0) == 1
        assert lib.adil_stem_bwd_variant(-1) == 0
    finally:
        lib.adil_stem_bwd_variant(first)
    assert first == 0 and lib.adil_stem_bwd_variant(-1) == 0     # the default is the new kernels


def test_refusals_come_before_any_launch_under_either_value():
    """The argument checks run before any device call, so they are reached on a machine without a GPU; the pointers are
    never followed."""
    _, lib = _bound()
    fake = ctypes.c_void_p(4096)
    one = ctypes.c_float(1.0)
    prev = lib.adil_stem_bwd_variant(-1)
    try:
        for variant in (0, 1):
            lib.adil_stem_bwd_variant(variant)
            for B, H, W, code in ((2, 3, 4, 0), (2, 4, 7, 1), (2, 4, 4, 2), (65536, 2, 2, 0), (0, 2, 2, 1)):
                assert lib.adil_stem_conv_bwd(fake, fake, one, one, one, fake, code, B, H, W, None) == -1, (variant, B, H, W, code)
            for B, OH, OW, C in ((2, 4, 4, 12), (2, 4, 4, 0), (0, 4, 4, 8), (2, 0, 4, 8), (2, 4, -2, 8)):
                assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, fake, B, OH, OW, C, None) == -1, (variant, B, OH, OW, C)
            assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, None, 2, 4, 4, 8, None) == -1
    finally:
        lib.adil_stem_bwd_variant(prev)
