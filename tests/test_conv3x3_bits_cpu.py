"""CPU: host side of the 3x3 convolution entry points after the loop switch (adil_conv3x3_loop) was retired: the built
library, the header's code and _lib.py no longer have the symbol, the product entry points keep their arguments under
ABI 8, and a weight pack of 2^31 elements or more (the kernel indexes the pack with 32 bits) is refused before any launch."""
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
    assert not hasattr(raw, "adil_conv3x3_loop")
    assert "adil_conv3x3_loop" not in code
    assert "adil_conv3x3_loop" not in _lib.SIGNATURES
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # the product calls stay as they were: nine arguments each
    for name in ("adil_conv3x3", "adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd"):
        assert hasattr(raw, name) and re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert len(_lib.SIGNATURES[name][1]) == 9, name


def test_weight_pack_of_two_to_the_31_elements_is_refused_without_a_launch():
    """The argument check runs before any device call, so it is reached on a machine without a GPU; the pointers are
    never followed."""
    _, lib = _bound()
    fake = ctypes.c_void_p(4096)
    # 9 * C * N: 15488^2 * 9 = 2 158 903 296 >= 2^31; 16384 * 14592 * 9 = 2^31 + 4 194 304
    for c, n in ((15488, 15488), (16384, 14592), (14592, 16384)):
        assert 9 * c * n >= 2 ** 31 and c % 64 == 0 and n % 64 == 0
        assert lib.adil_conv3x3(fake, fake, fake, 1, 1, 1, c, n, None) == -1, (c, n)
        assert lib.adil_conv3x3_s2_fwd(fake, fake, fake, 1, 2, 2, c, n, None) == -1, (c, n)
        assert lib.adil_conv3x3_s2_bwd(fake, fake, fake, 1, 2, 2, c, n, None) == -1, (c, n)
