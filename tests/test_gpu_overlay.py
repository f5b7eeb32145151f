"""efx_overlay (k_overlay.hip) on the device against tests/overlay_model.py, byte for byte, on padded regions whose fill
bytes must survive: the directed cases of tests/test_overlay_model.py (every alignment, sizes and positions, both kinds,
gains and fades, order, streams and pictures, invalid events among valid ones) with an atlas whose bytes between the
bitmaps differ from the model's, list lengths at the seams of the scan step, both strides, pieces against one long call,
every refused argument, and the Python methods up to make_title(overlays=)."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import overlay_model as M
import test_overlay_model as T
from test_gpu_telecine import Region

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
PICTURE = M.PICTURE
STEP = 256  # k_overlay's scan step (overlay_px.h: kScanStep)
CASES = T.cases()


@pytest.fixture(scope="module")
def efx():
    import espflix_amd
    espflix_amd.load_library()
    return espflix_amd


@pytest.fixture(scope="module")
def dec(efx):
    d = efx.Decoder(1, 1)
    yield d
    d.close()


def test_scan_step_is_the_kernels():
    """The list lengths below were chosen by this constant."""
    text = open(os.path.join(ROOT, "espflix_amd", "csrc", "overlay_px.h")).read()
    value = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", text).group(1))
    assert value("kScanStep") == STEP == 64 * value("kWaves") and "EFX_OVERLAY_MAX_EVENTS 4096" in open(os.path.join(ROOT, "include", "efx.h")).read()
    kernel = open(os.path.join(ROOT, "espflix_amd", "csrc", "k_overlay.hip")).read()
    assert "base += ovx::kScanStep" in kernel and "__launch_bounds__(ovx::kScanStep)" in kernel


def upload(dec, data, least=16):
    buf = dec.alloc(max(least, data.nbytes))
    if data.nbytes:
        buf.upload(data)
    return buf


def picture_region(dec, pictures, pad):
    """The streams of a call, a pad behind each."""
    n, P = pictures.shape[:2]
    reg = Region(dec, n, P * PICTURE, pad=pad)
    reg.expect(pictures.reshape(n, -1))
    reg.buf.upload(reg.want.reshape(-1))
    return reg


def status_region(dec, n):
    reg = Region(dec, 1, 4 * n)
    reg.expect(np.zeros((1, 4 * n), dtype=np.uint8))
    reg.buf.upload(reg.want.reshape(-1))
    return reg


def run_case(efx, dec, c, what, pad=64, with_status=True, want=None):
    """One call on padded regions against the model, whose atlas has other bytes between the bitmaps than the device's."""
    want = c.want(fill_seed=2) if want is None else want
    n = c.n_streams
    pics, st = picture_region(dec, c.pictures, pad), status_region(dec, n) if with_status else None
    ev, atlas = upload(dec, c.events), upload(dec, c.atlas(1))
    dec.overlay_to(pics.buf, ev if len(c.events) else None, atlas if len(c.events) else None, n_streams=n, n_pictures=c.n_pictures,
                   n_events=len(c.events), atlas_bytes=c.atlas_bytes, first_picture=c.first_picture, stride=pics.stride if pad else 0,
                   status=st.buf if st else None)
    dec.sync()
    pics.expect(want.reshape(n, -1))
    pics.check(what)
    if st:
        st.expect(np.full(n, M.status(c.events, c.atlas_bytes), dtype=np.uint32).view(np.uint8)[None, :])
        st.check((what, "status"))
        st.free()
    assert not len(c.events) or np.array_equal(ev.download(np.uint8, c.events.nbytes), c.events.view(np.uint8)), "the events were written"
    for b in (ev, atlas):
        b.free()
    pics.free()
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_directed_cases(efx, dec, name):
    c = CASES[name]
    want = run_case(efx, dec, c, name)
    if name == "outside":
        assert np.array_equal(want, c.pictures)
    if name == "invalid":
        assert M.status(c.events, c.atlas_bytes) == efx.OVERLAY_BAD_EVENT and not np.array_equal(want, c.pictures)
        run_case(efx, dec, c, "invalid events, no status words", with_status=False, want=want)


def test_order_reversed_differs(efx, dec):
    a, b = T.order(), T.order(reverse=True)
    wa, wb = a.want(), b.want()
    assert not np.array_equal(wa, wb), "the model's two orders agree: the case is vacuous"
    run_case(efx, dec, a, "order", want=wa)
    run_case(efx, dec, b, "order reversed", want=wb)


@pytest.mark.parametrize("n_streams,n_pictures", [(1, 1), (3, 5)])
def test_default_stride(efx, dec, n_streams, n_pictures):
    """stride = 0: the streams lie one behind the other."""
    run_case(efx, dec, T.streams(n_streams, n_pictures), ("stride 0", n_streams, n_pictures), pad=0)


def test_pictures_without_events_are_left_alone(efx, dec):
    c = T.streams(3, 5)
    want = run_case(efx, dec, c, "streams 3 x 5")
    assert np.array_equal(want[:, [1, 3]], c.pictures[:, [1, 3]]) and not np.array_equal(want[:, [0, 2, 4]], c.pictures[:, [0, 2, 4]])


@pytest.mark.parametrize("n", [0, 1, STEP - 1, STEP, STEP + 1, 4 * STEP + 1])
def test_list_lengths(efx, dec, n):
    """The shown events are the list's first and last; n = 0 launches nothing and returns EFX_OK."""
    c = T.listed(n)
    want = run_case(efx, dec, c, ("list of", n))
    assert (n == 0) == np.array_equal(want, c.pictures)


def test_pieces_equal_one_long_call(efx, dec):
    c = T.pieces()
    whole = run_case(efx, dec, c, "one long call")
    pics = picture_region(dec, c.pictures, 64)
    ev, atlas = upload(dec, c.events), upload(dec, c.atlas(1))
    kw = dict(n_streams=2, n_events=len(c.events), atlas_bytes=c.atlas_bytes, stride=pics.stride)
    dec.overlay_to(pics.buf, ev, atlas, n_pictures=5, first_picture=0, **kw)
    dec.overlay_to(pics.buf.ptr + 5 * PICTURE, ev, atlas, n_pictures=7, first_picture=5, **kw)
    dec.sync()
    pics.expect(whole.reshape(2, -1))
    pics.check("two pieces")
    for b in (ev, atlas):
        b.free()
    pics.free()


def test_argument_errors(efx, dec):
    """Every EFX_ERR_ARG case of include/efx.h returns its status and leaves the pictures alone."""
    lib = efx.load_library()
    c = T.kinds()
    n, P = 2, 3
    pictures = np.random.default_rng(40).integers(0, 256, (n, P, PICTURE), dtype=np.uint8)
    pics, st = picture_region(dec, pictures, 64), status_region(dec, n)
    ev, atlas = upload(dec, c.events), upload(dec, c.atlas(1))
    ok = dict(n_streams=n, n_pictures=P, n_events=len(c.events), reserved=0, first_picture=0, stride=pics.stride, atlas_bytes=c.atlas_bytes)

    def status(ep, ap, pp, sp, **kw):
        o = np.zeros(1, dtype=efx.OVERLAY_OPTS_DTYPE)
        for k, v in {**ok, **kw}.items():
            o[0][k] = v
        return lib.efx_overlay(dec._ctx, o.ctypes.data, ep, ap, pp, sp)

    E, A, Pp, S = ev.ptr, atlas.ptr, pics.buf.ptr, st.buf.ptr
    cases = [dict(n_streams=0), dict(n_streams=-1), dict(n_pictures=0), dict(n_pictures=-1), dict(n_events=-1), dict(n_events=4097),
             dict(n_streams=1 << 16, n_pictures=1 << 15, stride=(1 << 15) * PICTURE),   # 2^31 pictures
             dict(first_picture=-1), dict(first_picture=(1 << 40) - P + 1), dict(first_picture=1 << 40), dict(reserved=1),
             dict(stride=P * PICTURE - 16), dict(stride=pics.stride + 8), dict(stride=16)]
    for kw in cases:
        assert status(E, A, Pp, S, **kw) == ARG, kw
        assert lib.efx_last_error(dec._ctx).startswith(b"efx_overlay: "), kw
    for ep, ap, pp in [(E, A, None), (E, A, Pp + 8), (None, A, Pp), (E, None, Pp), (E + 4, A, Pp)]:
        assert status(ep, ap, pp, S) == ARG, (ep, ap, pp)
    assert lib.efx_overlay(dec._ctx, None, E, A, Pp, S) == ARG
    dec.sync()
    pics.check("after the refused calls")
    st.check("the status words after the refused calls")
    # what is accepted: the last title index, no events without a list or an atlas, no status words
    assert status(E, A, Pp, None, first_picture=(1 << 40) - P) == 0
    assert status(None, None, Pp, S, n_events=0) == 0 and status(None, None, Pp, None, n_events=0, atlas_bytes=0) == 0
    dec.sync()
    pics.check("calls that show nothing")
    assert status(E, A, Pp, S) == 0
    dec.sync()
    pics.expect(M.overlay(pictures, c.events, c.atlas(2), c.atlas_bytes).reshape(n, -1))
    pics.check("the accepted call")
    st.check("the status words of the accepted call")
    for b in (ev, atlas):
        b.free()
    pics.free()
    st.free()


def overlays_of(efx, c):
    """The Overlay list of a case without invalid records."""
    out = []
    for e, (offset, pitch, rows) in zip(c.events, c.placed):
        bitmap = rows.reshape(int(e["h"]), int(e["w"]), 4) if e["kind"] == M.RGBA else rows
        col = int(e["colour"])
        out.append(efx.Overlay(np.ascontiguousarray(bitmap), int(e["first"]), int(e["last"]), int(e["x"]), int(e["y"]),
                               colour=(col >> 16, col >> 8 & 255, col & 255), stream=int(e["stream"]), opacity=int(e["opacity"]),
                               fade_in=int(e["fade_in"]), fade_out=int(e["fade_out"])))
    return out


def test_overlay_on_arrays(efx, dec):
    """Decoder.overlay() on NumPy arrays: the model's pictures, a copy; pieces by first_picture; the ValueErrors."""
    c = T.pieces()
    ovs = overlays_of(efx, c)
    before = c.pictures.copy()
    out = dec.overlay(c.pictures, ovs)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == c.pictures.shape
    assert np.array_equal(out, c.want()) and np.array_equal(c.pictures, before)
    second = dec.overlay(c.pictures[:, 5:], ovs, first_picture=5)
    assert np.array_equal(second, c.want()[:, 5:])
    far = dec.overlay(c.pictures[:, :2], ovs, first_picture=100)  # no event can show: the pictures come back as they are
    assert np.array_equal(far, c.pictures[:, :2]) and far is not c.pictures
    assert np.array_equal(dec.overlay(c.pictures[:, :2], []), c.pictures[:, :2])
    f = T.fades()
    assert np.array_equal(dec.overlay(f.pictures, overlays_of(efx, f), first_picture=13), f.want())
    bad = efx.Overlay(ovs[0].bitmap, 30, 20, 0, 0)
    with pytest.raises(ValueError, match="event 1 "):
        dec.overlay(c.pictures[:, :4], [ovs[1], efx.Overlay(ovs[0].bitmap, 0, 3, 0, 0, stream=-2)])
    with pytest.raises(ValueError, match="event 2 "):
        dec.overlay(c.pictures[:, :4], [ovs[1], bad, efx.Overlay(ovs[0].bitmap, 0, 3, 5000, 0)])  # (bad can never show: it is dropped)
    with pytest.raises(ValueError):
        dec.overlay(c.pictures[0], ovs)
    with pytest.raises(ValueError):
        dec.overlay(c.pictures, ovs, inplace=True)
    with pytest.raises(efx.EfxError):
        dec.overlay_to(0, 0, 0, n_streams=1, n_pictures=1, n_events=1, atlas_bytes=16)


TORCH_CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    import torch  # (first: the HIP runtime of this process is torch's)
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, sys.argv[1] + "/tests")
    import espflix_amd as efx
    import overlay_model as M
    import test_overlay_model as T
    from test_gpu_overlay import overlays_of, title_inputs

    dec = efx.Decoder(3, 1, 2, device=torch.cuda.current_device(), max_stream_bytes=8 << 20)
    c = T.pieces()
    ovs, want = overlays_of(efx, c), c.want()
    t = torch.from_numpy(c.pictures).cuda()
    out = dec.overlay(t, ovs)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.data_ptr() != t.data_ptr()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), c.pictures)
    same = dec.overlay(t, ovs, inplace=True)
    assert same.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), want)
    try:
        dec.overlay(torch.from_numpy(c.pictures).cuda().transpose(0, 1).contiguous().transpose(0, 1), ovs, inplace=True)
        raise SystemExit("a tensor that is not packed was accepted in place")
    except ValueError:
        pass

    # make_title(overlays=) against make_title of pictures burnt beforehand; without overlays against the calls by hand
    pics, pcm, ovs = title_inputs(efx)
    kw = dict(speed=3, qscale=8, gop=6, search=3, first_pts=129003)
    burnt = dec.overlay(pics, ovs)
    assert not np.array_equal(burnt, pics)
    for src, bsrc, p in ((pics, burnt, pcm), (torch.from_numpy(pics).cuda(), torch.from_numpy(burnt).cuda(), torch.from_numpy(pcm).cuda())):
        a, st_a = dec.make_title(src, p, overlays=ovs, **kw)
        b, st_b = dec.make_title(bsrc, p, **kw)
        plain, st_p = dec.make_title(src, p, **kw)
        assert (st_a == 0).all() and (st_b == 0).all() and (st_p == 0).all() and len(a) == len(b) == 1
        assert sorted(a[0]) == ["video.idx", "video.ts", "video_fwd.ts", "video_rwd.ts"]
        for k in a[0]:
            assert a[0][k] == b[0][k], k
        assert all(a[0][k] != plain[0][k] for k in ("video.ts", "video_fwd.ts", "video_rwd.ts"))
        if not isinstance(src, np.ndarray):
            assert np.array_equal(src.cpu().numpy(), pics), "make_title changed the caller's pictures"
        none, st_n = dec.make_title(src, p, overlays=[], **kw)
        assert all(none[0][k] == plain[0][k] for k in plain[0])
        # the parent commit's path: encode_av, trick_streams, index_streams and idx_build by hand
        titles, st = dec.encode_av(src, p, fps=None, aq=None, qscale=8, gop=6, search=3, first_pts=129003)
        fwd, rwd, tst = dec.trick_streams(src, speed=3, gop=3, fps=None, aq=None, qscale=8, search=3, first_pts=129003)
        res = dec.index_streams([titles[0], fwd[0], rwd[0]], trick_speed=[1, 3, 3])
        idx = efx.idx_build([rec for rec, _ in res], [smp for _, smp in res])
        assert plain[0] == {"video.ts": titles[0], "video_fwd.ts": fwd[0], "video_rwd.ts": rwd[0], "video.idx": idx}
        assert np.array_equal(st_p, np.vstack([st[None], tst]))
    dec.close()
    print("overlay ok")
""")


def title_inputs(efx):
    """One stream of 12 pictures, a moving ramp with a little noise, 0.4 s of a 440 Hz tone, and a subtitle that fades
    over pictures 2 .. 9 with a logo on every picture."""
    rng = np.random.default_rng(50)
    pics = np.empty((1, 12, PICTURE), dtype=np.uint8)
    yy, xx = np.mgrid[0:M.H, 0:M.W]
    for k in range(12):
        pics[0, k, :M.CB] = ((xx + 3 * k) // 2 + yy // 3 + rng.integers(0, 3, (M.H, M.W))).clip(16, 235).reshape(-1)
        pics[0, k, M.CB:M.CR], pics[0, k, M.CR:] = 110 + k, 140 - k
    t = np.arange(19200)
    pcm = np.round(6000 * np.sin(2 * np.pi * 440 * t / 48000)).astype(np.int16)[None]
    ovs = [efx.Overlay(T.alpha(rng, 24, 301), 2, 9, 25, 160, fade_in=2, fade_out=3),
           efx.Overlay(T.rgba(rng, 24, 48), 0, 11, 296, 8, opacity=200)]
    return pics, pcm, ovs


def test_tensors_and_make_title(efx, tmp_path):
    """overlay() on tensors, in place and not, and make_title(overlays=) (a process of its own: torch's HIP runtime first)."""
    script = tmp_path / "overlay_tensor.py"
    script.write_text(TORCH_CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "overlay ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
