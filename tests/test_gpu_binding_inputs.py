"""The convenience methods of the Python binding take a NumPy array, an aligned contiguous tensor or a tensor whose address
is 8 mod 16 (staged by Decoder._stage): the three must give the same result, element for element, and leave the caller's
tensor as it was.  The array path of every method is held against its model elsewhere, so agreement is enough here.  One
error path: a tensor of the wrong dtype raises ValueError and the decoder works on.  The cases run in one child process
(torch's HIP runtime has to be this process's first), which reports every case; each is a test of its own."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["compare", "conform", "trick_streams", "encode", "encode_quality_recon", "deinterlace", "detelecine_info", "detect_crop",
         "import_pictures_auto_crop", "loudness", "normalize", "import_pcm", "sbc_encode", "encode_av", "wrong_dtype_unwinds"]

CHILD = textwrap.dedent("""
    import dataclasses, json, sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    import espflix_amd as efx

    PIC = efx.FRAME_BYTES
    rng = np.random.default_rng(2031)
    dec = efx.Decoder(2, 1, 2, device=torch.cuda.current_device())

    def forms(a):
        # the same data as an array, an aligned tensor and a tensor 8 bytes into a larger flat one
        aligned = torch.from_numpy(a).cuda()
        lead = 8 // a.itemsize
        big = torch.zeros(a.size + lead, dtype=aligned.dtype, device="cuda")
        off = big[lead:].view(a.shape)
        off.copy_(aligned)
        assert aligned.is_contiguous() and aligned.data_ptr() % 16 == 0 and off.is_contiguous() and off.data_ptr() % 16 == 8
        return a, aligned, off

    def plain(r):
        # a result as nested lists of arrays and bytes
        if isinstance(r, torch.Tensor):
            return r.cpu().numpy()
        if dataclasses.is_dataclass(r):
            return [plain(getattr(r, f.name)) for f in dataclasses.fields(r)]
        if isinstance(r, (list, tuple)):
            return [plain(v) for v in r]
        return r

    def same(a, b):
        if isinstance(a, list):
            return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, np.ndarray):
            return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and \\
                np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        return type(a) is type(b) and a == b

    report = {}

    def case(name, call, *inputs):
        # call(*inputs in one form) for each of the three forms
        try:
            results, notes = [], []
            for k in range(3):
                args = [forms(a)[k] for a in inputs]
                results.append(plain(call(*args)))
                if k and not all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(args, inputs)):
                    notes.append(f"form {k}: the caller's tensor changed")
            notes += [f"form {k} differs from the array's result" for k in (1, 2) if not same(results[0], results[k])]
            report[name] = notes
            return results[0]
        except Exception as e:
            report[name] = [f"{type(e).__name__}: {e}"]

    pics = rng.integers(0, 256, (2, 5, PIC), dtype=np.uint8)
    other = np.clip(pics.astype(np.int16) + rng.integers(-3, 4, pics.shape), 0, 255).astype(np.uint8)
    case("compare", lambda r, t: dec.compare(r, t, macroblocks=True), pics, other)
    case("conform", lambda p: dec.conform(p, 30, 24), pics)
    case("trick_streams", lambda p: dec.trick_streams(pictures=p, speed=2), pics)
    case("encode", lambda p: dec.encode(p), pics)
    case("encode_quality_recon", lambda p: dec.encode(p, quality=True, recon=True), pics)

    # 18 x 8 I420: 216 bytes an image, so the source and the destination rows pad to 224 and the crop-back runs
    W, H = 18, 8
    frames = rng.integers(0, 256, (2 * 6, W * H * 3 // 2), dtype=np.uint8)
    progressive = case("deinterlace", lambda f: dec.deinterlace(f, width=W, height=H, n_streams=2), frames)
    case("detelecine_info", lambda f: dec.detelecine(f, width=W, height=H, n_streams=2, info=True), frames)
    case("detect_crop", lambda f: dec.detect_crop(f, fmt="i420", width=W, height=H), frames[:3])
    case("import_pictures_auto_crop", lambda f: dec.import_pictures(f, fmt="i420", width=W, height=H, crop="auto"), frames[:3])

    pcm = rng.integers(-20000, 20000, (2, 6404), dtype=np.int16)  # over 400 ms at 16 kHz; 6404 is no multiple of 8
    case("loudness", lambda p: dec.loudness(p, 16000), pcm)
    case("normalize", lambda p: dec.normalize(p, 16000), pcm)
    case("import_pcm", lambda p: dec.import_pcm(p, rate=8000, out_rate=16000), pcm[:, :300].reshape(2, 100, 3).copy())
    case("sbc_encode", lambda p: dec.sbc_encode(p), pcm[:, :256].copy())
    case("encode_av", lambda v, p: dec.encode_av(v, p), pics[:, :2].copy(), pcm[:, :256].copy())

    # the error path: the scratch unwinds, the decoder works on
    try:
        notes = []
        try:
            dec.deinterlace(torch.zeros(frames.shape, dtype=torch.int16, device="cuda"), width=W, height=H, n_streams=2)
            notes.append("no ValueError for an int16 tensor")
        except ValueError:
            pass
        dec.sync()
        again = dec.deinterlace(frames, width=W, height=H, n_streams=2)
        if progressive is None or not np.array_equal(again, progressive):
            notes.append("the call after the error gives another answer")
        report["wrong_dtype_unwinds"] = notes
    except Exception as e:
        report["wrong_dtype_unwinds"] = [f"{type(e).__name__}: {e}"]
    dec.close()
    json.dump(report, open(sys.argv[2], "w"))
    print("binding inputs ran")
""")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("binding_inputs")
    script, out = tmp / "child.py", tmp / "report.json"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "binding inputs ran" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return json.load(open(out))


@pytest.mark.parametrize("name", CASES)
def test_array_tensor_and_misaligned_tensor_agree(report, name):
    assert report[name] == []


def test_every_case_is_listed(report):
    assert sorted(report) == sorted(CASES)
