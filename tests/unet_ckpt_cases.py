"""Broken and hostile checkpoint directories for the UNet's checkpoint reader (csrc/unet_ckpt.hip), shared by its two tests:
tests/test_unet_abi_cpu.py (through the ABI, ctypes) and tests/test_unet_ckpt_cpu.py (the stand-alone driver under
AddressSanitizer / UBSan).  Each generator rewrites the directory `d` in place and yields, once per case,
`(variant, substrings, what)`: the reader must fail on `d` with an error message that holds one of `substrings`."""
import json
import struct

CONFIG = dict(in_channels=8, out_channels=4, block_out_channels=[64, 128], num_attention_heads=[1, 2], layers_per_block=1,
              down_block_types=["CrossAttnDownBlockSpatioTemporal", "DownBlockSpatioTemporal"],
              up_block_types=["UpBlockSpatioTemporal", "CrossAttnUpBlockSpatioTemporal"])

BAD_ENTRIES = [
    {"dtype": "F16", "shape": [-1, 8, 3, 3], "data_offsets": [0, 16]},                       # negative dimension
    {"dtype": "F16", "shape": [1 << 40, 1 << 40], "data_offsets": [0, 16]},                  # product overflows 2^64
    {"dtype": "F16", "shape": [1 << 33, 1 << 33], "data_offsets": [0, 16]},                  # 2^66 elements
    {"dtype": "F16", "shape": [2.5, 8], "data_offsets": [0, 16]},                            # fractional
    {"dtype": "F16", "shape": [64, 8, 3, 3], "data_offsets": [-16, 16]},                     # negative offset
    {"dtype": "F16", "shape": [64, 8, 3, 3], "data_offsets": [0, 1e30]},                     # far beyond 2^53
    {"dtype": "F16", "shape": [1 << 30], "data_offsets": [0, 16]},                           # count x 2 != the 16 bytes it names
    {"dtype": "F16", "shape": [8] * 9, "data_offsets": [0, 16]},                             # too many dimensions
    {"dtype": "F16", "shape": "oops", "data_offsets": [0, 16]},
]
BAD_ENTRY_ERRORS = ("shape", "malformed", "outside the file", "size mismatch", "exceeds", "JSON", "missing tensor")

# raw headers json.dumps would not write: a truncated \u escape at the end, and a number that runs to the last header byte
RAW_HEADERS = (b'{"a\\u12', b'{"conv_in.weight":{"dtype":"F16","shape":[1],"data_offsets":[0,2', b'{"x":' + b"9" * 400)


def write_safetensors(path, header: dict, payload: bytes = b""):
    hb = json.dumps(header).encode()
    path.write_bytes(struct.pack("<Q", len(hb)) + hb + payload)


def broken_directories(d):
    """From an empty directory to a readable file that is not this model's: what is wrong with each, in the reader's order."""
    yield b"fp16", ("config.json",), "empty directory"
    (d / "config.json").write_text("{ not json")
    yield b"fp16", ("JSON",), "config.json is not JSON"
    (d / "config.json").write_text(json.dumps(dict(block_out_channels=[64, 100], num_attention_heads=[1, 2])))
    yield b"fp16", ("head dim",), "100 channels is not 64 x heads"
    cfg = dict(CONFIG, down_block_types=["CrossAttnDownBlockSpatioTemporal", "NoSuchBlock"])
    (d / "config.json").write_text(json.dumps(cfg))
    yield b"fp16", ("NoSuchBlock",), "unknown block type"
    (d / "config.json").write_text(json.dumps(CONFIG))
    yield b"fp16", ("safetensors",), "no weights file at all"
    (d / "diffusion_pytorch_model.fp16.safetensors").write_bytes(b"\x01\x02\x03")
    yield b"fp16", ("not a safetensors file",), "too short to hold a header"
    (d / "diffusion_pytorch_model.fp16.safetensors").unlink()
    st = d / "diffusion_pytorch_model.safetensors"
    write_safetensors(st, {"conv_in.weight": {"dtype": "F16", "shape": [64, 8, 3, 3], "data_offsets": [0, 9216]}})
    yield None, ("outside the file", "exceeds the file"), "the entry points past the end of the file"
    write_safetensors(st, {"conv_in.weight": {"dtype": "I8", "shape": [4], "data_offsets": [0, 4]}, "__metadata__": {"format": "pt"}}, b"\0" * 4)
    yield None, ("unsupported dtype",), "a dtype the reader does not convert"
    write_safetensors(st, {"conv_in.bias": {"dtype": "F32", "shape": [2], "data_offsets": [0, 8]}}, b"\0" * 8)
    yield None, ("missing tensor",), "a readable file that is not this model's"


def hostile_headers(d):
    """Dimensions, offsets and escapes of the safetensors header are file contents: negative / overflowing / fractional / huge
    values, a truncated \\u escape and a number at the very end of the header."""
    (d / "config.json").write_text(json.dumps(CONFIG))
    st = d / "diffusion_pytorch_model.safetensors"
    for ent in BAD_ENTRIES:
        write_safetensors(st, {"conv_in.weight": ent}, b"\0" * 16)
        yield None, BAD_ENTRY_ERRORS, ent
    for raw in RAW_HEADERS:
        st.write_bytes(struct.pack("<Q", len(raw)) + raw)
        yield None, ("JSON",), raw
    # a header length that covers the whole file (no payload) with a sane entry: outside the file, not a wrapped offset
    write_safetensors(st, {"conv_in.weight": {"dtype": "F16", "shape": [4], "data_offsets": [(1 << 52) - 8, (1 << 52)]}})
    yield None, ("outside the file",), "offsets near 2^52"
