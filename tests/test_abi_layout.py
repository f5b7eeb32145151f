"""espflix_amd/_abi.py is a mirror of include/efx.h: a C99 program over the header, built here with the host compiler,
prints sizeof of every struct and offsetof / size of every field the Python side names, and each ctypes.Structure and
record dtype is held against it.  A field added to the header and forgotten in Python fails here, not in a call.  No GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import espflix_amd as efx
from espflix_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRUCTS = {
    "_Config": "efx_config", "_VideoParams": "efx_video_params", "_FieldOpts": "efx_field_opts", "_ExportOpts": "efx_export_opts",
    "_ImportOpts": "efx_import_opts", "_CropOpts": "efx_crop_opts", "_Surface": "efx_surface", "_DeintOpts": "efx_deint_opts",
    "_DetelecineOpts": "efx_detelecine_opts", "_ImportColour": "efx_import_colour", "_ImportHdr": "efx_import_hdr",
    "_CompareOpts": "efx_compare_opts", "_CompareRec": "efx_compare_rec", "_TrickOpts": "efx_trick_opts",
    "_ConformOpts": "efx_conform_opts", "_EncodeOpts": "efx_encode_opts", "_EncodeRate": "efx_encode_rate",
    "_SceneCut": "efx_scene_cut", "_AdaptiveQuant": "efx_adaptive_quant", "_EncPictureInfo": "efx_enc_picture_info",
    "_SbcEncodeOpts": "efx_sbc_encode_opts", "_ImportPcmOpts": "efx_import_pcm_opts",
    "_LoudnessStepsOpts": "efx_loudness_steps_opts", "_LoudnessGateOpts": "efx_loudness_gate_opts",
    "_PcmGainOpts": "efx_pcm_gain_opts", "_MuxOpts": "efx_mux_opts", "_IdxRec": "efx_idx_rec", "_Timing": "efx_timing",
}
# the structs that arrive in arrays: the NumPy record dtype of each
DTYPES = {
    "LOUDNESS_STEP_DTYPE": "efx_loudness_step", "LOUDNESS_REC_DTYPE": "efx_loudness_rec", "TELECINE_INFO": "efx_telecine_info",
    "ENC_PICTURE_INFO_DTYPE": "efx_enc_picture_info",
}


def header_fields(c_name):
    """The field names of a struct of efx.h, read from its text (for the dtypes, whose names need not all coincide)."""
    hdr = open(os.path.join(ROOT, "include", "efx.h")).read()
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", "", hdr, flags=re.S)
    body = re.search(r"typedef struct " + c_name + r"\s*\{(.*?)\}\s*" + c_name + ";", hdr, flags=re.S).group(1)
    # "int32_t x, y;" and "uint64_t sse[3];": the last identifier of every declarator
    return [re.search(r"([A-Za-z_]\w*)\s*(\[[^\]]*\])?\s*$", part.strip()).group(1)
            for decl in body.split(";") for part in decl.split(",") if part.strip()]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """{c struct: (sizeof, {field: (offset, size)})} as the host C compiler lays efx.h out."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a host C compiler is needed to lay out include/efx.h"
    wanted = {c: [n for n, *_ in getattr(_abi, py)._fields_] for py, c in STRUCTS.items()}
    for py, c in DTYPES.items():
        wanted.setdefault(c, [n for n in getattr(_abi, py).names if n in header_fields(c)])
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "efx.h"', "int main(void) {"]
    for c, fields in wanted.items():
        lines.append(f'  printf("S {c} %zu\\n", sizeof({c}));')
        for f in fields:
            lines.append(f'  printf("F {c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c} *)0)->{f}));')
    lines += ["  return 0;", "}"]
    tmp = tmp_path_factory.mktemp("abi_layout")
    src, exe = tmp / "layout.c", tmp / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    sizes, fields = {}, {}
    for line in out.splitlines():
        w = line.split()
        if w[0] == "S":
            sizes[w[1]] = int(w[2])
        else:
            fields.setdefault(w[1], {})[w[2]] = (int(w[3]), int(w[4]))
    return {c: (sizes[c], fields.get(c, {})) for c in sizes}


def test_the_table_covers_every_structure_of_the_package():
    defined = {name for mod in (efx, _abi) for name, v in vars(mod).items()
               if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}
    assert defined == set(STRUCTS)
    assert len(STRUCTS) == 28 and len(set(STRUCTS.values())) == 28
    for name in list(STRUCTS) + list(DTYPES):
        assert getattr(efx, name) is getattr(_abi, name), f"espflix_amd.{name} is not the one of _abi.py"
    assert efx._SYMBOLS is _abi._SYMBOLS and efx._P is _abi._P


@pytest.mark.parametrize("py_name", sorted(STRUCTS))
def test_structure_matches_the_header(layout, py_name):
    cls = getattr(_abi, py_name)
    size, fields = layout[STRUCTS[py_name]]
    assert ctypes.sizeof(cls) == size
    assert [n for n, *_ in cls._fields_] == header_fields(STRUCTS[py_name]), "the header names other fields, or in another order"
    for name, *_ in cls._fields_:
        d = getattr(cls, name)
        assert (d.offset, d.size) == fields[name], f"{py_name}.{name}"


@pytest.mark.parametrize("py_name", sorted(DTYPES))
def test_record_dtype_matches_the_header(layout, py_name):
    dt = getattr(_abi, py_name)
    size, fields = layout[DTYPES[py_name]]
    assert dt.itemsize == size
    shared = [n for n in dt.names if n in fields]
    assert shared, "no field name coincides with the header's"
    for name in shared:
        sub, offset = dt.fields[name][:2]
        assert (offset, sub.itemsize) == fields[name], f"{py_name}.{name}"
    # packed: the fields cover the record, so a field the header has and the dtype lacks shows as a hole
    assert sum(dt.fields[n][0].itemsize for n in dt.names) == dt.itemsize
