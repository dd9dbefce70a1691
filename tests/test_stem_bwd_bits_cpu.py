"""CPU: host side of the stem backward entry points after their kernel switch (adil_stem_bwd_variant) was retired: the built
library, the header's code and _lib.py no longer have the symbol, the two product entry points keep their arguments under
ABI 8 and refuse what they refused, and the shapes beyond the kernels' grids, which once fell back to the retired
kernels, are refused as well."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound():
    from dl_attack_on_imagenet_amd import _lib
    from dl_attack_on_imagenet_amd.build import build_library
    build_library(verbose=False)
    return _lib, _lib.load()


def test_the_switch_is_gone_and_the_product_calls_are_as_they_were():
    _lib, bound = _bound()
    raw = ctypes.CDLL(_lib.LIBPATH)
    src = open(os.path.join(ROOT, "include", "adil_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert not hasattr(raw, "adil_stem_bwd_variant")
    assert "adil_stem_bwd_variant" not in code
    assert "adil_stem_bwd_variant" not in _lib.SIGNATURES
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # the product calls stay as they were
    for name, nargs in (("adil_stem_pool_bwd", 10), ("adil_stem_conv_bwd", 11)):
        assert hasattr(raw, name) and re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name


def test_refusals_come_before_any_launch():
    """The argument checks run before any device call, so they are reached on a machine without a GPU; the pointers are
    never followed."""
    _, lib = _bound()
    fake = ctypes.c_void_p(4096)
    one = ctypes.c_float(1.0)
    for B, H, W, code in ((2, 3, 4, 0), (2, 4, 7, 1), (2, 4, 4, 2), (65536, 2, 2, 0), (0, 2, 2, 1)):
        assert lib.adil_stem_conv_bwd(fake, fake, one, one, one, fake, code, B, H, W, None) == -1, (B, H, W, code)
    for B, OH, OW, C in ((2, 4, 4, 12), (2, 4, 4, 0), (0, 4, 4, 8), (2, 0, 4, 8), (2, 4, -2, 8)):
        assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, fake, B, OH, OW, C, None) == -1, (B, OH, OW, C)
    assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, None, 2, 4, 4, 8, None) == -1


def test_shapes_beyond_the_grids_are_refused_without_a_launch():
    """One past each limit of include/adil_hip.h: B * PH = 2^31 rows of quads; 65536 workgroups along a row; 65535 x 32896
    tiles of 32 x 16 input pixels."""
    _, lib = _bound()
    fake = ctypes.c_void_p(4096)
    one = ctypes.c_float(1.0)
    B, OH, OW, C = 65536, 65535, 2, 8
    assert B * ((OH - 1) // 2 + 1) == 2 ** 31
    assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, fake, B, OH, OW, C, None) == -1
    B, OH, OW, C = 1, 1, 2, 134215688
    assert C % 8 == 0 and -(-((OW - 1) // 2 + 1) * (C // 8) // 256) == 65536
    assert lib.adil_stem_pool_bwd(fake, fake, fake, fake, fake, B, OH, OW, C, None) == -1
    B, H, W = 65535, 2048, 8224
    assert B * -(-H // 16) * -(-W // 32) == 65535 * 32896 > 2 ** 31 - 1
    for code in (0, 1):
        assert lib.adil_stem_conv_bwd(fake, fake, one, one, one, fake, code, B, H, W, None) == -1, code
