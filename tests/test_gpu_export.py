"""efx_export_frames (k_export): ring frames out as I420 / RGB24 / RGBP on the device, against the reference's frame
hashes and, bit for bit, against the NumPy model of include/efx.h's formulas (tests/export_model.py)."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import common
import export_model as M
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB_CASES = [(fmt, chroma, full) for fmt in ("rgb24", "rgbp") for chroma in ("nearest", "bilinear") for full in (False, True)]


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


def decoder(efx, streams, fmt, max_pictures, ring_depth=None, groups=None):
    dec = efx.Decoder(max_streams=len(streams), max_pictures=max_pictures, ring_depth=ring_depth or max_pictures + 1,
                      max_stream_bytes=sum(len(s) for s in streams) + 4096)
    if groups:
        dec.set_option(efx.OPT_GROUPS, groups)
    dec.upload(streams, fmt)
    dec.decode()
    return dec


def fnv_strips_of_i420(i420):
    from espflix_amd import gen
    strips = M.i420_to_strip(i420.reshape(-1, M.FRAME_BYTES))
    return [gen.fnv1a64(strips[k]) for k in range(strips.shape[0])]


def download_at(dec, buf, offset, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    assert offset + nbytes <= buf.nbytes
    st = dec._lib.efx_memcpy_d2h(dec._ctx, out.ctypes.data, buf.ptr + offset, nbytes)
    assert st == 0
    return out


@pytest.mark.parametrize("clip", ["splash", "vmedia"])
def test_i420_repacks_to_the_reference_frames(efx, clip, clips, golden):
    """Every picture of the embedded clips exported as I420 (picture mode), re-packed to the strip layout on the host:
    the FNV-1a-64 of each is the hash the unmodified reference left for that picture."""
    want = golden["clips"][clip]["hashes"]
    dec = decoder(efx, [clips[clip]], efx.FORMAT_TS, 100)
    n = dec.picture_count(0)
    assert dec.stream_status(0) == 0 and n == len(want)
    got = []
    for p in range(n):
        img = dec.export_host("i420", picture=p)
        assert img.shape == (1, M.FRAME_BYTES)
        got += fnv_strips_of_i420(img)
    assert [f"{h:016x}" for h in got] == want
    dec.close()


@pytest.mark.parametrize("source", ["clips", "synthetic"])
def test_rgb_bit_exact_against_the_model(efx, clips, source):
    from espflix_amd import gen
    if source == "clips":
        streams, fmt, P = [clips["splash"], clips["vmedia"]], efx.FORMAT_TS, 100
        pictures = [0, 1, 17, 40, 63]
    else:
        streams, fmt, P = gen.Batch(0, 24, 12, 12, 0, threads=16).all_es(), efx.FORMAT_ES, 12
        pictures = [0, 5, 11]
    dec = decoder(efx, streams, fmt, P)
    n = len(streams)
    for p in pictures:
        frames = np.stack([dec.download_frame(s, dec.picture_slot(p, s)) for s in range(n)])
        for fmt_, chroma, full in RGB_CASES:
            got = dec.export_host(fmt_, picture=p, chroma=chroma, full_range=full)
            want = M.export(frames, fmt_, chroma, full)
            assert got.shape == want.shape
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"picture {p} {fmt_} {chroma} full_range={full}: first difference at {bad[0].tolist()}"
        assert np.array_equal(dec.export_host("i420", picture=p), M.strip_to_i420(frames))
    dec.close()


def cb_cr_es(dc_cb: int, dc_cr: int) -> bytes:
    """One intra picture written bit by bit: DC-only macroblocks, luma DC 128, block 4 (Cb) DC 128 + dc_cb and block 5
    (Cr) DC 128 + dc_cr (the differential on the first macroblock of each slice, the prediction carries it on)."""
    from espflix_amd import gen
    head = gen.Batch(0, 1, 1, 12, 0, threads=1).es(0).tobytes()
    head = head[:head.index(b"\x00\x00\x01\x00")]  # sequence + GOP header of a generator stream
    b = common._Bits()
    b.start_code(0x00)
    b.put(0, 10)       # temporal_reference
    b.put(1, 3)        # I picture
    b.put(0xFFFF, 16)  # vbv_delay
    b.put(0, 1)        # extra_bit_picture

    def chroma_dc(d):
        if d == 0:
            b.put(0b00, 2)
            return
        size = abs(d).bit_length()
        assert size >= 2  # (size 1 is spelled 01)
        b.put((1 << size) - 2, size)  # table B-13: size 2 -> 10, 3 -> 110, ... (size ones, then a zero)
        b.put(d if d > 0 else d + (1 << size) - 1, size)

    for row in range(12):
        b.start_code(row + 1)
        b.put(8, 5)    # quantizer_scale
        b.put(0, 1)    # extra_bit_slice
        for col in range(22):
            b.put(1, 1)        # macroblock_address_increment 1
            b.put(1, 1)        # macroblock_type: intra
            for _ in range(4):
                b.put(0b100, 3)  # luma dct_dc_size 0
                b.put(0b10, 2)   # end_of_block
            chroma_dc(dc_cb if col == 0 else 0)
            b.put(0b10, 2)
            chroma_dc(dc_cr if col == 0 else 0)
            b.put(0b10, 2)
    b.start_code(0xB7)
    return head + bytes(b.out)


def test_cb_cr_plane_mapping(efx):
    """Block 4 (Cb) lifted, block 5 (Cr) lowered: U must come out above 128 and V below it -- swapped planes fail."""
    es = np.frombuffer(cb_cr_es(40, -40), dtype=np.uint8)
    n, h, _, _ = oracle.decode(es, 0)
    assert n == 1
    dec = decoder(efx, [es], efx.FORMAT_ES, 1, 2)
    assert dec.stream_status(0) == 0 and dec.picture_count(0) == 1
    slot = dec.picture_slot(0)
    assert int(dec.frame_hashes()[0, slot]) == int(h[0])
    y, u, v = efx.i420_planes(dec.export_host("i420", picture=0)[0])
    assert u.shape == v.shape == (96, 176)
    assert (u > 128).all() and (v < 128).all()
    for chroma in ("nearest", "bilinear"):
        rgb = dec.export_host("rgb24", picture=0, chroma=chroma)[0].astype(int)
        assert (rgb[..., 2] > rgb[..., 0]).all()
    dec.close()


def test_picture_mode_equals_slot_mode(efx):
    """Streams in different ring slots for the same picture index: late PES PTS (no buffer swap before it), unequal
    picture counts, three reconstruction groups, two calls so that the ring positions drift apart."""
    from espflix_amd import gen
    streams = []
    for k in range(32):
        es = gen.Batch(k, 1, 12 - (k % 5), 12, 0, threads=1).es(0).tobytes()
        streams.append(np.frombuffer(common.late_pts_ts(es, k % 4) if k % 3 == 0 else common.one_pes_per_picture(es),
                                     dtype=np.uint8))
    P = 12
    dec = efx.Decoder(max_streams=32, max_pictures=P, ring_depth=P + 1, max_stream_bytes=2 * sum(len(s) for s in streams))
    dec.set_option(efx.OPT_GROUPS, 3)
    for call in range(2):
        dec.upload(streams if call == 0 else streams[::-1], efx.FORMAT_TS)
        dec.decode()
    counts = [dec.picture_count(s) for s in range(32)]
    assert len(set(counts)) > 1
    slots = np.array([[dec.picture_slot(p, s) for s in range(32)] for p in range(P)])
    assert any(len(set(slots[p])) > 1 for p in range(P))       # streams disagree on the slot of a picture
    assert any((slots[p] != (p + 1) % (P + 1)).any() for p in range(P))
    for p in range(P):
        got = dec.export_host("i420", picture=p)
        by_slot = np.stack([dec.export_host("i420", slot=int(slots[p, s]), first_stream=s, n_streams=1)[0] for s in range(32)])
        assert np.array_equal(got, by_slot), f"picture {p}"
        want = M.strip_to_i420(np.stack([dec.download_frame(s, int(slots[p, s])) for s in range(32)]))
        assert np.array_equal(got, want)
        sub = dec.export_host("rgbp", picture=p, first_stream=5, n_streams=20, chroma="bilinear")
        assert np.array_equal(sub, M.export(M.i420_to_strip(want[5:25]), "rgbp", "bilinear"))
    dec.close()


def test_no_sync_pipeline(efx):
    """Five upload -> decode -> picture-mode export calls queued back to back (more calls than hand-over slots, two
    groups each), one sync: every buffer holds its own call's picture."""
    from espflix_amd import gen
    S, P, calls = 16, 6, 5
    batches = [gen.Batch(100 * c, S, P - (c % 3), 12, 0, threads=16).all_es() for c in range(calls)]
    pics = [(c * 2) % (P - (c % 3)) for c in range(calls)]

    ref = efx.Decoder(max_streams=S, max_pictures=P, ring_depth=2)
    ref.set_option(efx.OPT_GROUPS, 2)
    want = []
    for c in range(calls):
        ref.upload(batches[c], efx.FORMAT_ES)
        ref.decode()
        frames = np.stack([ref.download_frame(s, ref.picture_slot(pics[c], s)) for s in range(S)])
        want.append(M.export(frames, "rgb24", "bilinear"))
    ref.close()

    dec = efx.Decoder(max_streams=S, max_pictures=P, ring_depth=2)
    dec.set_option(efx.OPT_GROUPS, 2)
    bufs = [dec.alloc(S * M.RGB_BYTES) for _ in range(calls)]
    for c in range(calls):
        dec.upload(batches[c], efx.FORMAT_ES)
        dec.decode(sync=False)
        dec.export_to(bufs[c], "rgb24", n_streams=S, picture=pics[c], chroma="bilinear")
    dec.sync()
    for c in range(calls):
        got = bufs[c].download(np.uint8, S * M.RGB_BYTES).reshape(want[c].shape)
        assert np.array_equal(got, want[c]), f"call {c}"
        bufs[c].free()
    dec.close()


def test_strides_and_errors(efx):
    from espflix_amd import gen
    S, P = 8, 4
    dec = efx.Decoder(max_streams=S + 4, max_pictures=P, ring_depth=3)
    lib, ctx = dec._lib, dec._ctx

    def call(ptr, first=0, n=S, slot=-1, picture=0, fmt=efx.PIX_RGB24, chroma=efx.CHROMA_BILINEAR, full=0, stride=0):
        o = efx._ExportOpts(first, n, slot, picture, fmt, chroma, full, stride)
        return lib.efx_export_frames(ctx, C.byref(o), ptr)

    buf = dec.alloc((S + 4) * (M.RGB_BYTES + 64))
    # before any decode: slot mode works, picture mode is a state error
    assert call(buf.ptr, slot=0) == 0
    assert call(buf.ptr) == -5
    dec.upload(gen.Batch(0, S, P, 12, 0, threads=16).all_es(), efx.FORMAT_ES)
    dec.decode()
    ARG, STATE = -1, -5
    assert call(None) == ARG
    assert call(buf.ptr + 8) == ARG
    assert call(buf.ptr, fmt=3) == ARG and call(buf.ptr, fmt=-1) == ARG
    assert call(buf.ptr, chroma=2) == ARG and call(buf.ptr, fmt=efx.PIX_RGBP, chroma=-1) == ARG
    assert call(buf.ptr, fmt=efx.PIX_I420, chroma=7) == 0  # chroma is ignored for I420
    assert call(buf.ptr, stride=M.RGB_BYTES - 16) == ARG and call(buf.ptr, stride=M.RGB_BYTES + 8) == ARG
    assert call(buf.ptr, first=-1) == ARG and call(buf.ptr, n=0) == ARG and call(buf.ptr, first=5, n=S) == ARG
    assert call(buf.ptr, slot=3) == ARG and call(buf.ptr, slot=-2) == ARG
    assert call(buf.ptr, picture=-1) == ARG and call(buf.ptr, picture=P) == ARG
    assert call(buf.ptr, first=4, n=S) == STATE        # inside max_streams, beyond the decoded batch
    assert call(buf.ptr, first=4, n=S, slot=1) == 0    # slot mode reads any stream of the ring
    assert lib.efx_export_bytes(3) == 0 and lib.efx_export_bytes(efx.PIX_RGBP) == M.RGB_BYTES
    dec.sync()

    # a stride larger than the image: the gaps keep what was there
    for fmt, code, image in (("rgb24", efx.PIX_RGB24, M.RGB_BYTES), ("i420", efx.PIX_I420, M.FRAME_BYTES)):
        stride = image + 48
        n = S - 2
        buf.upload(np.full(buf.nbytes, 0xA5, dtype=np.uint8))
        assert call(buf.ptr, first=1, n=n, picture=P - 1, fmt=code, stride=stride) == 0
        dec.sync()
        raw = buf.download(np.uint8, buf.nbytes)
        frames = np.stack([dec.download_frame(s, dec.picture_slot(P - 1, s)) for s in range(1, 1 + n)])
        want = M.export(frames, fmt, "bilinear").reshape(n, -1)
        for i in range(n):
            assert np.array_equal(raw[i * stride:i * stride + image], want[i])
            assert (raw[i * stride + image:(i + 1) * stride] == 0xA5).all()
        assert (raw[n * stride:] == 0xA5).all()
    buf.free()
    with pytest.raises(ValueError):
        dec.export_host("yuv444")
    with pytest.raises(efx.EfxError):
        dec.export_host("rgb24", slot=3)
    dec.close()


TORCH_CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    import espflix_amd as efx
    from espflix_amd import gen

    S, P = 12, 5
    # a stream of torch's own (the default stream's handle is 0, which tells the library to make a private one)
    torch.cuda.set_stream(torch.cuda.Stream())
    dec = efx.Decoder(S, P, ring_depth=P + 1, device=torch.cuda.current_device(),
                      hip_stream=torch.cuda.current_stream().cuda_stream)
    dec.upload(gen.Batch(7, S, P, 12, 0, threads=16).all_es(), efx.FORMAT_ES)
    dec.decode(sync=False)
    checked = 0
    for fmt, shape in (("rgb24", (S, 192, 352, 3)), ("rgbp", (S, 3, 192, 352)), ("i420", (S, 101376))):
        for chroma in ("nearest", "bilinear"):
            out = torch.full((S * efx.export_bytes(fmt),), 7, dtype=torch.uint8, device="cuda")
            t = dec.export(fmt, picture=P - 1, chroma=chroma, out=out, sync=False)  # ordered on torch's stream
            assert tuple(t.shape) == shape and t.data_ptr() == out.data_ptr()
            got = t.cpu().numpy()
            assert np.array_equal(got, dec.export_host(fmt, picture=P - 1, chroma=chroma)), (fmt, chroma)
            checked += 1
    t = dec.export("i420", picture=1, full_range=True)  # allocated by export(), synchronised
    y, u, v = efx.i420_planes(t)
    assert tuple(y.shape) == (S, 192, 352) and tuple(u.shape) == (S, 96, 176) and tuple(v.shape) == (S, 96, 176)
    assert np.array_equal(t.cpu().numpy(), dec.export_host("i420", picture=1))
    for bad in (torch.empty(S * 202752, dtype=torch.int16, device="cuda"), torch.empty(S * 202752 + 1, dtype=torch.uint8, device="cuda"),
                torch.empty(S * 202752, dtype=torch.uint8), torch.empty((S * 202752, 2), dtype=torch.uint8, device="cuda")[:, 0]):
        try:
            dec.export("rgb24", picture=0, out=bad)
        except ValueError:
            checked += 1
    dec.close()
    print("torch export ok", checked)
""")


def test_torch_tensor_out(efx, tmp_path):
    """In a child process (torch's HIP runtime must come up first): a decoder on torch's current stream, export() into a
    preallocated tensor without a sync, equal to export_host; out= checks."""
    script = tmp_path / "torch_export.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "torch export ok 10" in r.stdout


def test_batch_of_2048_streams(efx):
    from espflix_amd import gen
    S, P = 2048, 4
    b = gen.Batch(0, S, P, 12, 0, threads=16)
    streams = b.all_es()
    b.close()
    dec = efx.Decoder(max_streams=S, max_pictures=P, ring_depth=2)
    dec.upload(streams, efx.FORMAT_ES)
    dec.decode()
    p = P - 1
    slots = np.array([dec.picture_slot(p, s) for s in range(S)])

    buf = dec.alloc(S * M.RGB_BYTES)
    dec.export_to(buf, "rgb24", picture=p, chroma="bilinear")
    dec.sync()
    for s in np.random.default_rng(5).choice(S, 64, replace=False):
        got = download_at(dec, buf, int(s) * M.RGB_BYTES, M.RGB_BYTES).reshape(192, 352, 3)
        want = M.export(dec.download_frame(int(s), int(slots[s])), "rgb24", "bilinear")
        assert np.array_equal(got, want), f"stream {s}"

    dec.export_to(buf, "i420", picture=p)
    dec.sync()
    i420 = buf.download(np.uint8, S * M.FRAME_BYTES).reshape(S, M.FRAME_BYTES)
    buf.free()
    got = fnv_strips_of_i420(i420)
    hashes = dec.frame_hashes()
    assert got == [int(hashes[s, slots[s]]) for s in range(S)]
    dec.close()
