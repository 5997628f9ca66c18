"""CPU tier of the single-call UNet ABI (csrc/unet.hip) and, through it, of the checkpoint reader (csrc/unet_ckpt.hip): the
reader's error paths - every one of them ends before the first device call, so no GPU is needed.  The broken directories live
in tests/unet_ckpt_cases.py; tests/test_unet_ckpt_cpu.py runs the reader alone on the same ones under AddressSanitizer / UBSan."""
import ctypes as C

import pytest

from unet_ckpt_cases import broken_directories, hostile_headers


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib
    return _lib.load()


def _create(lib, d, variant=b"fp16"):
    h = C.c_void_p()
    rc = lib.syn3r_unet_create(str(d).encode(), variant, C.byref(h))
    return rc, lib.syn3r_last_error().decode(), h


def test_unet_create_reports_what_is_wrong_with_a_directory(lib, tmp_path):
    for variant, substrings, what in broken_directories(tmp_path):
        rc, err, _ = _create(lib, tmp_path, variant=variant)
        assert rc != 0 and any(k in err for k in substrings), (what, err)


def test_unet_handles_are_checked(lib):
    junk = (C.c_char * 4096)()
    assert lib.syn3r_unet_workspace_bytes(C.cast(junk, C.c_void_p), 1, 2, 8, 8, 1) == 0
    assert lib.syn3r_unet_destroy(C.cast(junk, C.c_void_p)) != 0 and b"live handle" in lib.syn3r_last_error()
    assert lib.syn3r_unet_destroy(None) == 0


def test_unet_create_survives_hostile_safetensors_headers(lib, tmp_path):
    """Dimensions, offsets and escapes of the header are file contents: negative / overflowing / fractional / huge values, a
    truncated \\u escape and a number at the very end of the header must end in an error return (never an exception through
    extern "C", an allocation sized by the header, or a read past the mapping)."""
    for variant, substrings, what in hostile_headers(tmp_path):
        rc, err, h = _create(lib, tmp_path, variant=variant)
        assert rc != 0 and not h.value, what
        assert any(k in err for k in substrings), (what, err)
