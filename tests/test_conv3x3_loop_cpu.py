"""CPU: host side of the 3x3 convolution's loop switch (adil_conv3x3_loop): the built library exports the symbol, the
header declares it and _lib.py binds it under ABI 8; the switch keeps the contract of adil_pw_route_policy; a weight pack of
2^31 elements or more (the kernel indexes the pack with 32 bits) is refused before any launch."""
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
    assert hasattr(raw, "adil_conv3x3_loop")
    assert re.search(r"\bint\s+adil_conv3x3_loop\s*\(\s*int\s+\w+\s*\)\s*;", code)
    restype, argtypes = _lib.SIGNATURES["adil_conv3x3_loop"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_int]
    assert bound.adil_abi_version() == _lib.ABI_VERSION == 8
    # the product calls stay as they were: nine arguments each
    for name in ("adil_conv3x3", "adil_conv3x3_s2_fwd", "adil_conv3x3_s2_bwd"):
        assert len(_lib.SIGNATURES[name][1]) == 9, name


def test_switch_returns_the_previous_value_and_ignores_other_arguments():
    _, lib = _bound()
    first = lib.adil_conv3x3_loop(1)
    try:
        assert lib.adil_conv3x3_loop(0) == 1
        assert lib.adil_conv3x3_loop(1) == 0
        for other in (2, -1, 7, 1 << 30):
            assert lib.adil_conv3x3_loop(other) == 1             # a query: nothing changes
        assert lib.adil_conv3x3_loop(0) == 1
        assert lib.adil_conv3x3_loop(-1) == 0
    finally:
        lib.adil_conv3x3_loop(first)
    assert first == 0 and lib.adil_conv3x3_loop(-1) == 0         # the default is the new loop


def test_weight_pack_of_two_to_the_31_elements_is_refused_without_a_launch():
    """The argument check runs before any device call, so it is reached on a machine without a GPU; the pointers are
    never followed."""
    _, lib = _bound()
    fake = ctypes.c_void_p(4096)
    prev = lib.adil_conv3x3_loop(-1)
    try:
        for variant in (0, 1):
            lib.adil_conv3x3_loop(variant)
            # 9 * C * N: 15488^2 * 9 = 2 158 903 296 >= 2^31; 16384 * 14592 * 9 = 2^31 + 4 194 304
            for c, n in ((15488, 15488), (16384, 14592), (14592, 16384)):
                assert 9 * c * n >= 2 ** 31 and c % 64 == 0 and n % 64 == 0
                assert lib.adil_conv3x3(fake, fake, fake, 1, 1, 1, c, n, None) == -1, (variant, c, n)
                assert lib.adil_conv3x3_s2_fwd(fake, fake, fake, 1, 2, 2, c, n, None) == -1, (variant, c, n)
                assert lib.adil_conv3x3_s2_bwd(fake, fake, fake, 1, 2, 2, c, n, None) == -1, (variant, c, n)
    finally:
        lib.adil_conv3x3_loop(prev)
