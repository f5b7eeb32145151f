"""Video for the multiplexer's tests, written packet by packet: PID-0x100 transport streams made from a list of units, and
the families of cases tests/test_mux_model.py (the model alone) and tests/test_gpu_mux_edges.py (the device against the
model) both run.  k_mux.hip reads packet headers and PES starts only, so the payload is filler -- different in every packet,
so that a packet in the wrong place shows.  Every case carries its own coverage assertion: from the model's unit list and
plain arithmetic it asserts that the condition the case aims at occurs, so a change here cannot quietly empty a case."""
import functools
from collections import namedtuple

import numpy as np

import mux_model as X

MASK33 = (1 << 33) - 1

# One PES.  packets: how many; pts: None = PTS_DTS_flags clear; af: adaptation_field_length of the start packet (None = no
# adaptation field); prefix False: the payload begins 00 00 02; no_payload: the start packet has adaptation_field_control 2;
# cont_af: adaptation_field_length of every second continuation packet.
Unit = namedtuple("Unit", "packets pts af prefix no_payload cont_af", defaults=(1, None, None, True, False, None))


def build(units, seed=0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    out, cc = [], 0
    for u in units:
        for k in range(u.packets):
            p = rng.integers(0, 256, 188, dtype=np.uint8)
            start = k == 0
            af = u.af if start else (u.cont_af if k % 2 else None)
            afc = 3 if af is not None else 1
            if start and u.no_payload:
                afc, af = 2, 183
            p[:4] = [0x47, (0x40 if start else 0) | 0x01, 0x00, (afc << 4) | (cc & 15)]
            cc += 1
            off = 4
            if af is not None:
                p[4] = af
                p[5:min(188, 5 + af)] = 0xFF
                if af:
                    p[5] = 0x00
                off = 5 + af
            if start and not u.no_payload:
                has = u.pts is not None
                hdr = bytes([0, 0, 1 if u.prefix else 2, 0xE0, 0, 0, 0x80, 0x80 if has else 0, 5 if has else 0])
                hdr += X.pts_bytes(u.pts) if has else b""
                n = max(0, min(len(hdr), 188 - off))
                p[off:off + n] = np.frombuffer(hdr[:n], dtype=np.uint8)
            out.append(p)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def blank(video: np.ndarray, fill: int = 0x00) -> np.ndarray:
    """The stream with one value in place of the filler: the same packets and PES starts to the multiplexer.  For the
    reference player, which decodes the video it demultiplexes: its decoder skips zero bits up to the next start code, so a
    payload of zeros takes it to the end of the stream, where it pauses.  Any other payload it reads as start codes four
    bytes at a time -- the random filler as pictures and slices, and a constant one leaves it aligned with the end code only
    when the payload's length happens to be a multiple of four; otherwise it reads past the end of its input and waits."""
    pk = video.copy().reshape(-1, 188)
    for p in pk:
        afc = (p[3] >> 4) & 3
        off = 4 + (1 + int(p[4]) if afc & 2 else 0)
        if p[1] & 0x40 and afc & 1 and off + 9 <= 188:
            off += 9 + (5 if p[off + 7] & 0x80 else 0)
        p[min(off, 188):] = fill
    return pk.reshape(-1)


def spread(t0, t1, n_units, seed, max_packets=3):
    """n_units PES with PTS from t0 to t1, one to max_packets packets each."""
    rng = np.random.default_rng(seed)
    return [Unit(int(rng.integers(1, max_packets + 1)), int(t)) for t in np.linspace(t0, t1, n_units).astype(np.int64)]


def r16(v):
    return (v + 15) // 16 * 16


class Case:
    """One launch: videos side by side, n_frames frames of fb bytes each, opt = the keywords of Decoder.mux_to."""

    def __init__(self, name, videos, fb, n_frames, opt=None, dst_stride=None, cover=None, names=None, same_frames=False):
        """names: the streams' names, for the coverage assertion.  same_frames: every stream gets stream 0's frames, so that
        the model runs once per distinct video of a batch that repeats its videos."""
        self.name, self.videos, self.fb, self.n_frames, self.dst_stride = name, videos, fb, n_frames, dst_stride
        self.opt = dict(opt or {})
        self.names = names
        self._cover = cover
        seed = sum(name.encode()) * 131 + fb
        self.frames = np.random.default_rng(seed).integers(0, 256, size=(len(videos), n_frames * fb), dtype=np.uint8)
        if same_frames:
            self.frames[:] = self.frames[0]
        self._same_frames = same_frames
        self._model = None

    @property
    def fpp(self):
        return self.opt.get("frames_per_pes", 8)

    @property
    def n_pes(self):
        return -(-self.n_frames // self.fpp)

    def pes_pts(self, j):
        """The PTS of audio PES j before it is masked to 33 bits."""
        o = self.opt
        return X.audio_pts(o.get("audio_first_frame", 0) + j * self.fpp, o.get("audio_first_pts", 0), o.get("samples_per_frame", 128),
                           o.get("sample_rate", 48000))

    def model_one(self, video, frames, **over):
        o = dict(self.opt, **over)
        return X.mux(video, frames, frame_bytes=self.fb, frames_per_pes=o.get("frames_per_pes", 8), pid=o.get("audio_pid", 0x101),
                     spf=o.get("samples_per_frame", 128), rate=o.get("sample_rate", 48000), first_pts=o.get("audio_first_pts", 0),
                     first_frame=o.get("audio_first_frame", 0), cc=o.get("audio_cc", 0), dst_stride=self.dst_stride, want_units=True)

    def model(self):
        """[(title, status, units)] per stream, from tests/mux_model.py."""
        if self._model is None:
            memo, self._model = {}, []
            for i, v in enumerate(self.videos):
                key = id(v) if self._same_frames else i
                if key not in memo:
                    memo[key] = self.model_one(v, self.frames[i])
                self._model.append(memo[key])
        return self._model

    def cover(self):
        """The condition this case aims at occurs: from the model alone."""
        res = self.model()
        if self._cover:
            self._cover(self, res)
        return res


def audio_units(units):
    return [u for u in units if u[0] == "a"]


def packet(title: bytes, k: int) -> bytes:
    return title[k * 188:(k + 1) * 188]


# ---- a. stuffing lengths ---------------------------------------------------------------------------------------------
#           fb  fpp frames cc   (14 + fpp x fb) mod 184 / the short last PES's
STUFFING = [(170, 1, 20, 15),   # 0: no adaptation field in the last packet
            (169, 1, 20, 3),    # 183: one byte of stuffing, adaptation_field_length 0
            (168, 1, 20, 0),    # 182: two
            (171, 1, 21, 14),   # 1: 183 bytes of stuffing
            (172, 1, 19, 7),    # 2
            (85, 4, 22, 5),     # the last PES holds 2 frames: 14 + 170 = 184
            (169, 2, 11, 12),   # the last PES holds 1 frame: 183
            (1, 1, 30, 0), (1, 32, 70, 9), (2048, 1, 5, 9), (9, 32, 70, 13), (524, 3, 10, 11),
            (64, 8, 1, 15),     # one frame
            (64, 8, 5, 2)]      # fewer frames than a PES holds


def residues(fb, fpp, n_frames):
    """(a full PES's, the short last PES's or None): (14 + payload) mod 184."""
    rest = n_frames % fpp
    return ((14 + fpp * fb) % 184 if n_frames >= fpp else None), ((14 + rest * fb) % 184 if rest else None)


def _cover_stuffing(case, res):
    title, st, units = res[0]
    assert st == 0
    au = audio_units(units)
    assert len(au) == case.n_pes
    for j, (_, _, first, n) in enumerate(au):
        n_fr = min(case.fpp, case.n_frames - j * case.fpp)
        r = (14 + n_fr * case.fb) % 184
        last = packet(title, first + n - 1)
        afc = (last[3] >> 4) & 3
        assert (afc == 1) if r == 0 else (afc == 3 and last[4] == 184 - r - 1), (case.name, j, r)


def stuffing():
    full = {residues(fb, fpp, n)[0] for fb, fpp, n, _ in STUFFING}
    short = {residues(fb, fpp, n)[1] for fb, fpp, n, _ in STUFFING}
    assert {0, 183, 182, 1, 2} <= full and {0, 183} <= short
    assert any(n == 1 for _, _, n, _ in STUFFING) and any(1 < n < fpp for _, fpp, n, _ in STUFFING)
    cases = []
    for k, (fb, fpp, n, cc) in enumerate(STUFFING):
        t0, dur = 5000, n * 240
        video = build(spread(t0 - 100, t0 + dur + 100, 12, seed=k), seed=100 + k)
        cases.append(Case(f"stuff_fb{fb}_fpp{fpp}_n{n}", [video, video[:0]], fb, n,
                          dict(frames_per_pes=fpp, audio_first_pts=t0, audio_cc=cc, audio_pid=0x101 + k % 2), cover=_cover_stuffing))
    # the counter wraps inside a PES: 12 packets a PES from counter 9, nine from 11
    for c in cases:
        if c.fb in (2048, 524):
            title, _, units = c.model()[0]
            assert any((packet(title, f)[3] & 15) + n - 1 >= 16 for _, _, f, n in audio_units(units)), c.name
    return cases


# ---- b. the PTS formula ----------------------------------------------------------------------------------------------
def around_ties(case, js, seed):
    """Video at one below, at and one above the PTS of the audio PES js."""
    units = []
    for j in js:
        p = case.pes_pts(j)
        units += [Unit(1, p - 1), Unit(2, p), Unit(1, p + 1)]
    return build(units, seed)


def _cover_ties(case, res):
    title, st, units = res[0]
    assert st == 0
    pattern = 0
    for k in range(len(units) - 3):
        a, b, c, d = units[k:k + 4]
        pattern += (a[0], b[0], c[0], d[0]) == ("v", "a", "v", "v") and a[1] == b[1] - 1 and b[1] == c[1] and d[1] == c[1] + 1
    assert pattern >= 3, (case.name, pattern)  # audio first at a tie, not before the video one tick earlier
    _, _, units1 = res[1]
    assert sum(u[0] == "a" and v[0] == "v" and u[1] == v[1] for u, v in zip(units1, units1[1:])) >= 3


def pts_formula():
    cases = []
    for spf in (32, 64, 96, 128):
        for rate in (16000, 32000, 44100, 48000):
            opt = dict(frames_per_pes=3, audio_first_frame=7, audio_first_pts=1234, samples_per_frame=spf, sample_rate=rate,
                       audio_cc=(spf // 32 + rate // 100) & 15)
            c = Case(f"pts_spf{spf}_rate{rate}", [None, None, None], 21, 50, opt, cover=_cover_ties)
            c.videos = [around_ties(c, range(1, 17, 2), seed=spf + rate),
                        build([u for j in range(0, 17, 2) for u in (Unit(2, c.pes_pts(j)), Unit(1))], seed=spf),
                        build([], 0)]
            if rate == 44100:  # the floor matters: the exact PTS of most PES is no whole number
                assert sum(((7 + 3 * j) * spf * 90000) % rate != 0 for j in range(c.n_pes)) > c.n_pes // 2
            cases.append(c)
    # the product (audio_first_frame + frame) x samples_per_frame x 90000 needs 64 bits, the PTS stays below 2^33
    opt = dict(frames_per_pes=7, audio_first_frame=30_000_000, audio_first_pts=777, audio_cc=4)
    c = Case("pts_first_frame_30e6", [None, None], 16, 41, opt, cover=_cover_ties)
    assert 30_000_000 % 7 and 30_000_000 * 128 * 90000 > 1 << 48
    assert 1 << 32 < c.pes_pts(0) and c.pes_pts(c.n_pes - 1) < 1 << 33
    c.videos = [around_ties(c, range(0, 6), seed=1), build([u for j in range(6) for u in (Unit(2, c.pes_pts(j)), Unit(1))], seed=2)]
    cases.append(c)
    return cases


# ---- c. video shapes ---------------------------------------------------------------------------------------------------
def shapes_video(T, D, seed=7):
    """D: ticks of one audio PES.  The PTS written in a start that must not be read lies far ahead: reading it would pull
    twenty-odd audio PES in front of that packet."""
    return build([
        Unit(2), Unit(1), Unit(3),                            # PTS-less before the first PTS
        Unit(2, T + D + 5), Unit(1, T + 3 * D),
        Unit(2), Unit(1),                                     # PTS-less in the middle
        Unit(2, T + 6 * D + 1),
        Unit(1, T + 2 * D), Unit(2, T + 4 * D),               # decreasing: the maximum so far holds
        Unit(1, T + 8 * D + 7),
        Unit(2, T + 10 * D, af=0), Unit(2),
        Unit(2, T + 12 * D, af=1), Unit(1),
        Unit(2, T + 14 * D, af=169), Unit(1),                 # the PTS ends with the packet
        Unit(1, T + 40 * D, af=170), Unit(1, T + 15 * D),     # a good start, the PTS runs out of the packet
        Unit(1, T + 41 * D, af=174), Unit(1, T + 16 * D),
        Unit(1, T + 42 * D, af=175), Unit(1, T + 17 * D),     # not a PES start
        Unit(2, T + 43 * D, no_payload=True), Unit(2, T + 18 * D),
        Unit(2, T + 44 * D, prefix=False), Unit(3, T + 19 * D, cont_af=7),
        Unit(4, T + 20 * D, af=3, cont_af=0), Unit(2, T + 22 * D)], seed)


def _cover_shapes(case, res):
    title, st, units = res[0]
    assert st == 0
    vu = X.video_units(case.videos[0])
    pts = [u[2] for u in vu]
    assert pts[:3] == [None] * 3 and pts[3] is not None and pts[5:7] == [None, None]
    assert any(a is not None and b is not None and b < a for a, b in zip(pts, pts[1:]))
    pk = case.videos[0].reshape(-1, 188)
    af = {int(pk[u[0], 4]): u[2] for u in vu if (pk[u[0], 3] >> 4) & 3 == 3}
    assert {0, 1, 169} <= {k for k, v in af.items() if v is not None} and {170, 174, 175} <= {k for k, v in af.items() if v is None}
    assert any((pk[u[0], 3] >> 4) & 3 == 2 and u[2] is None for u in vu)
    assert any((pk[u[0], 3] >> 4) & 3 == 1 and pk[u[0], 6] == 2 and u[2] is None for u in vu)
    assert any((pk[i, 3] >> 4) & 3 == 3 and not pk[i, 1] & 0x40 for i in range(len(pk)))
    au = [u[1] for u in audio_units(units)]
    assert au == sorted(au) and len(set(au)) == len(au)
    # audio lies between the video units, and what is later than the last video PES follows it
    kinds = "".join(u[0] for u in units)
    assert "va" in kinds.rstrip("a") and kinds.endswith("aaa")


def video_shapes():
    T, D = 10000, 480
    opt = dict(frames_per_pes=2, audio_first_pts=T, audio_cc=6)
    return [Case("video_shapes", [shapes_video(T, D), shapes_video(T + 3, D, seed=8), build([], 0)], 33, 120, opt, cover=_cover_shapes)]


# ---- d. chunk seams of pass 1 ------------------------------------------------------------------------------------------
SEAM_T, SEAM_D, SEAM_FRAMES = 50000, 240, 600
SEAM_END = SEAM_T + SEAM_FRAMES * SEAM_D


def seam_stream(n_pkts, t0, t1, seed, pts_of=None):
    """n_pkts packets in PES of 1 to 3, PES starts at packets 255 and 256, every fifth PES without PTS; pts_of(first packet,
    0..1 position in the stream) overrides the straight line from t0 to t1."""
    rng = np.random.default_rng(seed)
    sizes, at = [], 0
    while at < n_pkts:
        n = int(rng.integers(1, 4))
        for seam in (255, 256):
            if at < seam < at + n:
                n = seam - at
        n = min(n, n_pkts - at)
        sizes.append(n)
        at += n
    units, at = [], 0
    for k, n in enumerate(sizes):
        x = at / max(1, n_pkts - 1)
        pts = pts_of(at, x) if pts_of else int(t0 + (t1 - t0) * x)
        units.append(Unit(n, None if k % 5 == 4 and at not in (255, 256) else pts))
        at += n
    return build(units, seed)


def _front(units, video, packet_no):
    """Audio PES right in front of the video PES that starts at video packet packet_no."""
    first_of, at = {}, 0
    for k, u in enumerate(units):
        if u[0] == "v":
            first_of[at] = k
            at += u[3]
    k, n = first_of[packet_no], 0
    while k - n - 1 >= 0 and units[k - n - 1][0] == "a":
        n += 1
    return n


def _cover_seams(case, res):
    names = case.names
    for i, (title, st, units) in enumerate(res):
        assert st == 0, names[i]
    sizes = [v.size // 188 for v in case.videos[:7]]
    assert sizes == [1, 255, 256, 257, 512, 513, 799]
    for i in (3, 4, 5, 6):
        starts = {u[0]: u[2] for u in X.video_units(case.videos[i])}
        assert starts.get(255) is not None and starts.get(256) is not None
        kinds = "".join(u[0] for u in res[i][2])
        assert kinds.count("va") > 20  # interleaved all the way
    # the largest PTS in the first chunk, every later chunk lower
    vu = X.video_units(case.videos[names.index("max_first")])
    top = max((u for u in vu if u[2] is not None), key=lambda u: u[2])
    assert top[0] < 256 and case.videos[names.index("max_first")].size // 188 > 512
    assert all(u[2] < top[2] for u in vu if u[0] >= 256 and u[2] is not None) and sum(u[0] >= 256 and u[2] is not None for u in vu) > 50
    assert SEAM_T + 256 * SEAM_D < top[2] < SEAM_END  # audio behind it that only the carry keeps behind the later video
    i = names.index("jump_front")
    assert _front(res[i][2], case.videos[i], 0) > 256
    i = names.index("jump_later")
    assert _front(res[i][2], case.videos[i], 300) > 256
    kinds = "".join(u[0] for u in res[names.index("audio_later")][2])
    assert kinds.rstrip("a").count("a") == 0 and kinds.count("a") == SEAM_FRAMES and kinds[0] == "v"
    kinds = "".join(u[0] for u in res[names.index("audio_earlier")][2])
    assert kinds.startswith("a" * SEAM_FRAMES) and "a" not in kinds[SEAM_FRAMES:] and kinds.endswith("v")
    assert case.videos[names.index("no_video")].size == 0


def seam_videos():
    T, E, D = SEAM_T, SEAM_END, SEAM_D
    named = [(f"p{n}", seam_stream(n, T - 500, E + 500, seed=n)) for n in (1, 255, 256, 257, 512, 513, 799)]
    named += [
        ("max_first", seam_stream(600, 0, 0, 11, lambda at, x: T + 300 * D + 11 if at == 100 else int(T + 100 + x * 250 * D))),
        ("jump_front", seam_stream(300, T + 300 * D + 17, E + 100, 12)),
        ("jump_later", seam_stream(600, 0, 0, 13, lambda at, x: int(T - 4000 + 3000 * x) if at < 300 else int(T + 300 * D + (x - 0.5) * 500 * D))),
        ("audio_later", seam_stream(300, 1000, T - 1, 14)),
        ("audio_earlier", seam_stream(300, E, E + 90000, 15)),
        ("no_video", build([], 0))]
    return named


def seams():
    named = seam_videos()
    assert any(u[0] == 300 for u in X.video_units(dict(named)["jump_later"]))
    opt = dict(frames_per_pes=1, audio_first_pts=SEAM_T, audio_cc=1)
    c = Case("seams", [v for _, v in named], 8, SEAM_FRAMES, opt, cover=_cover_seams, names=[n for n, _ in named])
    def copied(case, res):
        for (title, st, units), v in zip(res, case.videos):
            assert st == 0 and title == v.tobytes() and all(u[0] == "v" for u in units)

    return [c, Case("no_audio", [v for _, v in named], 8, 0, opt, cover=copied)]


# ---- e. statuses -------------------------------------------------------------------------------------------------------
def rejected_videos():
    T, E = SEAM_T, SEAM_END
    far = []
    for k, (at, what) in enumerate(((300, "sync"), (400, "pid_101"), (500, "pid_1100"))):
        v = seam_stream(600, T, E, seed=20 + k)
        if what == "sync":
            v[at * 188] = 0x46
        elif what == "pid_101":
            v[at * 188 + 2] = 0x01
        else:
            v[at * 188 + 1] |= 0x10  # PID 0x1100: the low thirteen bits' upper five are 0x11, not 0x01
        far.append((f"bad_{what}_at_{at}", v))
    good = spread(T, T + 20 * SEAM_D, 10, seed=30)
    first = [("first_not_a_start", build([Unit(2, T)] + good, 31)[188:]),
             ("first_af_175", build([Unit(1, T, af=175)] + good, 32)),
             ("first_not_000001", build([Unit(1, T, prefix=False)] + good, 33))]
    return far + first


def _cover_statuses(case, res):
    for name, (title, st, _) in zip(case.names, res):
        bad = name.startswith(("bad_", "first_"))
        assert (st == X.MUX_BAD_VIDEO and title == b"") if bad else st == 0, name
    assert sum(r[1] != 0 for r in res) == 6
    for name, v in zip(case.names, case.videos):
        if name.startswith("bad_"):
            at = int(name.rsplit("_", 1)[1])
            assert at > 256 and X.video_units(v[:at * 188]) is not None and X.video_units(v[:(at + 1) * 188]) is None
        if name.startswith("first_"):
            assert X.video_units(v[:188]) is None and X.video_units(v[188:]) is not None


def statuses():
    bad = rejected_videos()
    good = [("good%d" % k, seam_stream(n, SEAM_T, SEAM_T + 100 * SEAM_D, seed=40 + k)) for k, n in enumerate((40, 300, 17, 1, 270, 90, 5))]
    named = [x for pair in zip(good, bad) for x in pair] + good[len(bad):]
    opt = dict(frames_per_pes=1, audio_first_pts=SEAM_T, audio_cc=8)
    c = Case("statuses", [v for _, v in named], 8, 100, opt, cover=_cover_statuses, names=[n for n, _ in named])
    # EFX_MUX_FULL at the exact boundary: a total that is a multiple of 16 fits a dst_stride equal to it, not 16 bytes less
    video = seam_stream(31, SEAM_T, SEAM_T + 30 * SEAM_D, seed=50)
    total = video.size + X.audio_packets(33, 8, 1) * 188
    assert total % 16 == 0

    def fits(case, res):
        assert [r[1] for r in res] == [0, 0] and len(res[0][0]) == total == case.dst_stride

    def full(case, res):
        assert [r[1] for r in res] == [X.MUX_FULL, 0] and res[0][0] == b"" and case.dst_stride == total - 16

    opt = dict(frames_per_pes=1, audio_first_pts=SEAM_T, audio_cc=15)
    return [c, Case("exactly_fits", [video, video[:188 * 7]], 8, 33, opt, dst_stride=total, cover=fits),
            Case("16_bytes_short", [video, video[:188 * 7]], 8, 33, opt, dst_stride=total - 16, cover=full)]


# ---- f. every shape side by side -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(n):
    """n streams of all the shapes above in one launch, rejected ones and ones that do not fit between good ones."""
    named = [("shapes", shapes_video(SEAM_T, SEAM_D))]
    seam, bad = seam_videos(), rejected_videos()
    for k, s in enumerate(seam):
        named.append(s)
        if k < len(bad):
            named.append(bad[k])
    named = [named[k % len(named)] for k in range(n)]
    stride = r16((650 + SEAM_FRAMES) * 188)  # the streams of more than 650 video packets do not fit

    def cover(case, res):
        st = [r[1] for r in res]
        if n > 1:
            assert {0, X.MUX_FULL, X.MUX_BAD_VIDEO} == set(st)
            assert any(a != 0 and b == 0 and c != 0 for a, b, c in zip(st, st[1:], st[2:]))
            assert any(a == 0 and b != 0 and c == 0 for a, b, c in zip(st, st[1:], st[2:]))
        else:
            assert st == [0]

    return Case(f"batch{n}", [v for _, v in named], 8, SEAM_FRAMES, dict(frames_per_pes=1, audio_first_pts=SEAM_T, audio_cc=1, audio_pid=0x102),
                dst_stride=stride, cover=cover, names=[nm for nm, _ in named], same_frames=True)


# ---- the PTS wrap ------------------------------------------------------------------------------------------------------
def wrap():
    """audio_first_pts = 2^33 - 20 000: the video's PTS are compared as written (33 bits), the audio's before they are masked,
    so the audio PES from the wrap on count as later than all video and follow the last video PES."""
    first = (1 << 33) - 20000
    D = 960
    opt = dict(frames_per_pes=4, audio_first_pts=first, audio_cc=3)
    units = [Unit(2, (first + k * 3003) & MASK33) for k in range(14)]
    video = build(units, seed=60)

    def cover(case, res):
        title, st, u = res[0]
        assert st == 0
        vp = [x.pts for x in units]
        assert sum(p > 1 << 32 for p in vp) >= 6 and sum(p < 30000 for p in vp) >= 6  # video on both sides of the wrap
        au = audio_units(u)
        n_before = sum(p < 1 << 33 for _, p, _, _ in au)
        assert 10 < n_before < len(au) - 10
        # the audio from the wrap on lies behind the last video PES, and its written PTS is masked
        last_video = max(k for k, x in enumerate(u) if x[0] == "v")
        assert all(k > last_video for k, x in enumerate(u) if x[0] == "a" and x[1] >= 1 << 33)
        assert any(x[0] == "v" and x[1] < 30000 for x in u[:last_video + 1])  # ... video whose PTS, unwrapped, is later than theirs
        for _, p, f, _ in au:
            assert packet(title, f)[4 + 9:4 + 14] == X.pts_bytes(p & MASK33)
            t = packet(title, f)[13:18]
            assert (((t[0] >> 1) & 7) << 30 | t[1] << 22 | (t[2] >> 1) << 15 | t[3] << 7 | t[4] >> 1) == p & MASK33 < 1 << 33

    return [Case("pts_wrap", [video, video[:188 * 8]], 64, 200, opt, cover=cover)]


@functools.lru_cache(maxsize=None)
def families():
    """Every family's cases, built once per process."""
    return {"stuffing": stuffing(), "pts": pts_formula(), "video": video_shapes(), "seams": seams(), "statuses": statuses(),
            "wrap": wrap()}
