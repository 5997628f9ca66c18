"""The UNet's checkpoint reader (csrc/unet_ckpt.hip) alone, on the CPU: built as plain C++ with AddressSanitizer + UBSan into
tests/unet_ckpt_driver.cpp and run as a child process - no HIP is linked and nothing is loaded into Python.
 * the broken and hostile directories of tests/unet_ckpt_cases.py (the ones test_unet_abi_cpu.py sends through the ABI): exit 1
   with the same error text, and no sanitizer report - a read past the header slice of the mapping stays inside the mapped page
   and goes unnoticed without one;
 * pack equality: every kernel-side layout the reader builds equals, bit for bit, what the Python host (model.py:_pack, ops.pack_*)
   builds from the same checkpoint - the two hosts are edited in lock-step, and this is where drift shows without a GPU."""
import json
import math
import os
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from unet_ckpt_cases import broken_directories, hostile_headers  # noqa: E402


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and Path(c).exists():
            return c
    return None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = tmp_path_factory.mktemp("ckpt_driver") / "unet_ckpt_driver"
    # host code only (-x c++: no device pass at all); -fno-gpu-sanitize says so to the driver as well, as in test_abi_sanitize.py
    san = ["-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined"]
    r = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", *san,
                        str(ROOT / "syn3r_amd" / "csrc" / "unet_ckpt.hip"), str(ROOT / "tests" / "unet_ckpt_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, d, variant, dump=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(d), variant.decode() if variant else "-"] + ([str(dump)] if dump else []),
                       capture_output=True, text=True, env=env, timeout=300)
    assert "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r


@pytest.mark.parametrize("cases", [broken_directories, hostile_headers])
def test_reader_refuses_broken_and_hostile_directories_cleanly(driver, tmp_path, cases):
    for variant, substrings, what in cases(tmp_path):
        r = _run(driver, tmp_path, variant)
        assert r.returncode == 1, (what, r.returncode, r.stdout, r.stderr[-2000:])
        assert any(k in r.stdout for k in substrings), (what, r.stdout)


# ------------------------------------------------------------------------------------------------ pack equality
def _read_dump(path):
    """The record format at the top of tests/unet_ckpt_driver.cpp."""
    buf = Path(path).read_bytes()
    pos = 0

    def take(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, buf, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def name():
        nonlocal pos
        n = take("I")
        pos += n
        return buf[pos - n:pos].decode()

    packs, alpha, slices = {}, {}, {}
    for _ in range(take("I")):
        k = name()
        rows, cols, n = take("qqQ")
        assert k not in packs, k
        packs[k] = (rows, cols, torch.from_numpy(np.frombuffer(buf, dtype="<i2", count=n, offset=pos).copy()))
        pos += 2 * n
    for _ in range(take("I")):
        k = name()
        alpha[k] = take("dd")
    for _ in range(take("I")):
        k = name()
        slices[k] = take("ii")
    assert pos == len(buf)
    return packs, alpha, slices


def _is_flattening(shape, rows, cols):
    """[rows, cols] is `shape` with its leading dimensions merged into rows and the rest into cols."""
    return any(math.prod(shape[:i]) == rows and math.prod(shape[i:]) == cols for i in range(len(shape) + 1))


CONFIGS = {
    # levels 64 / 128 / 128 / 128: geglu_w / geglu_b, geglu_w64 / geglu_b64, the padded conv_in / conv_out, _up4, qkv, the stacked time_emb_proj
    "pipeline": lambda UW: dict(UW.PIPELINE_CONFIG),
    # a C = 320 level (geglu_cw / geglu_cb) beside a 64-channel one, attention on the outer level only
    "c320": lambda UW: dict(UW.PIPELINE_CONFIG, block_out_channels=(320, 64), num_attention_heads=(5, 1), cross_attention_dim=64,
                            down_block_types=("CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"),
                            up_block_types=("UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal")),
}


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def checkpoint(request):
    """(name, the Python host with the checkpoint loaded and packed, its state dict in fp16): built once, read-only."""
    from oracle import unet_weights as UW
    from syn3r_amd.unet.model import UNetSpatioTemporalConditionModel
    model = UNetSpatioTemporalConditionModel(**CONFIGS[request.param](UW))
    sd = {k: v.to(torch.float16) for k, v in UW.make_state_dict(model.parameter_shapes(), seed=3).items()}
    model.load_state_dict(sd, "cpu")
    return request.param, model, sd


def _write_dir(d, model, sd, dtype, variant):
    from safetensors.torch import save_file
    d.mkdir()
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in model.config.items()}
    (d / "config.json").write_text(json.dumps(dict(cfg, _class_name="UNetSpatioTemporalConditionModel")))
    name = f"diffusion_pytorch_model.{variant}.safetensors" if variant else "diffusion_pytorch_model.safetensors"
    save_file({k: v.to(dtype).contiguous() for k, v in sd.items()}, str(d / name))


def _check_against_python_host(model, sd, dump):
    packs, alpha, slices = _read_dump(dump)
    for k, t in model.packed.items():                                     # every kernel-side layout of model.py:_pack
        assert k in packs, k
        rows, cols, bits = packs[k]
        assert _is_flattening(tuple(t.shape), rows, cols), (k, tuple(t.shape), rows, cols)
        assert torch.equal(t.contiguous().view(torch.int16).reshape(-1), bits), k
    stored = [k for k in sd if k not in model.packed and not k.endswith("mix_factor")]
    for k in stored:                                                       # everything else: as stored
        assert k in packs, k
        rows, cols, bits = packs[k]
        assert _is_flattening(tuple(sd[k].shape), rows, cols), (k, tuple(sd[k].shape), rows, cols)
        assert torch.equal(sd[k].contiguous().view(torch.int16).reshape(-1), bits), k
    assert set(packs) == set(model.packed) | set(stored), sorted(set(packs) ^ (set(model.packed) | set(stored)))[:8]
    assert alpha == model.alpha                                            # exactly: both are fp16 values held in doubles
    assert {k for k in sd if k.endswith("mix_factor")} == set(alpha) and alpha
    assert slices == model._temb_slices and slices


def test_packs_equal_the_python_host(driver, tmp_path, checkpoint):
    name, model, sd = checkpoint
    _write_dir(tmp_path / "f16", model, sd, torch.float16, "fp16")
    r = _run(driver, tmp_path / "f16", b"fp16", tmp_path / "f16.bin")
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    _check_against_python_host(model, sd, tmp_path / "f16.bin")
    if name != "pipeline":
        return
    # The two conversion branches, from the fp16-rounded values; no .fp16 file in these directories, so the plain name is found.
    # F32 holds every fp16 value exactly: the same dump is expected.  BF16 keeps 8 of fp16's 11 significant bits, so the file
    # holds bf16(v) and the expectation is what `.to(torch.float16)` makes of it - the Python host packed from those values.
    _write_dir(tmp_path / "f32", model, sd, torch.float32, None)
    r = _run(driver, tmp_path / "f32", b"fp16", tmp_path / "f32.bin")
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert (tmp_path / "f32.bin").read_bytes() == (tmp_path / "f16.bin").read_bytes()
    sd_bf = {k: v.to(torch.bfloat16).to(torch.float16) for k, v in sd.items()}
    assert any(not torch.equal(sd_bf[k], sd[k]) for k in sd)
    host_bf = type(model)(**model.config).load_state_dict(sd_bf, "cpu")
    _write_dir(tmp_path / "bf16", model, sd_bf, torch.bfloat16, None)
    r = _run(driver, tmp_path / "bf16", b"fp16", tmp_path / "bf16.bin")
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    _check_against_python_host(host_bf, sd_bf, tmp_path / "bf16.bin")
