"""The A/V multiplexer's output predicted in Python from the rules of include/efx.h (efx_mux_av): what k_mux.hip must write,
byte for byte, and the parsing helpers of the multiplexer tests."""
import numpy as np

MUX_FULL, MUX_BAD_VIDEO = 1024, 2048
PES_HDR = 14


def pts_bytes(pts: int) -> bytes:
    pts &= (1 << 33) - 1
    return bytes([0x21 | ((pts >> 29) & 0x0E), (pts >> 22) & 0xFF, 0x01 | ((pts >> 14) & 0xFE), (pts >> 7) & 0xFF,
                  0x01 | ((pts << 1) & 0xFE)])


def packets(pes: bytes, pid: int, cc: int) -> bytes:
    """A PES in 188-byte packets: payload_unit_start on the first, the last padded with adaptation-field stuffing."""
    out = bytearray()
    n = (len(pes) + 183) // 184
    for k in range(n):
        chunk = pes[k * 184:(k + 1) * 184]
        hdr = bytearray([0x47, (0x40 if k == 0 else 0) | (pid >> 8), pid & 0xFF, 0x10 | ((cc + k) & 15)])
        if len(chunk) < 184:
            stuff = 184 - len(chunk)
            hdr[3] |= 0x20
            hdr += bytes([stuff - 1]) + (b"\x00" + b"\xFF" * (stuff - 2) if stuff > 1 else b"")
        out += hdr + chunk
    return bytes(out)


def audio_pts(j_frame: int, first_pts: int, spf: int, rate: int) -> int:
    return first_pts + j_frame * spf * 90000 // rate


def video_units(ts: np.ndarray):
    """[(first packet, packets, PTS or None)] of the PES of a PID-0x100 transport stream; None if it is not one."""
    ts = np.asarray(ts, dtype=np.uint8)
    if ts.size % 188:
        return None
    pk = ts.reshape(-1, 188)
    units = []
    for i, p in enumerate(pk):
        if p[0] != 0x47 or (int(p[1]) & 0x1F) != 1 or p[2] != 0:
            return None
        start = bool(p[1] & 0x40)
        if i == 0 and not start:
            return None
        if start:
            afc = (int(p[3]) >> 4) & 3
            off = 4 + (1 + int(p[4]) if afc & 2 else 0)
            ok = bool(afc & 1) and off + 9 <= 188 and tuple(p[off:off + 3]) == (0, 0, 1)
            if i == 0 and not ok:
                return None
            pts = None
            if ok and (p[off + 7] & 0x80) and off + PES_HDR <= 188:
                t = [int(v) for v in p[off + 9:off + 14]]
                pts = ((t[0] >> 1) & 7) << 30 | t[1] << 22 | (t[2] >> 1) << 15 | t[3] << 7 | t[4] >> 1
            units.append([i, 1, pts])
        else:
            units[-1][1] += 1
    return units


def audio_packets(n_frames: int, fb: int, fpp: int) -> int:
    full, rest = divmod(n_frames, fpp)
    return full * ((PES_HDR + fpp * fb + 183) // 184) + ((PES_HDR + rest * fb + 183) // 184 if rest else 0)


def mux(video, frames, *, frame_bytes, frames_per_pes=8, pid=0x101, spf=128, rate=48000, first_pts=0, first_frame=0, cc=0,
        dst_stride=None, want_units=False):
    """(title bytes, status) for one stream; frames: the SBC frames back to back.  With want_units also the list of units as
    (kind 'v' / 'a', PTS, first output packet, packets)."""
    video = np.asarray(video, dtype=np.uint8)
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1)
    n_frames = frames.size // frame_bytes
    units = video_units(video)
    if units is None:
        return (b"", MUX_BAD_VIDEO, []) if want_units else (b"", MUX_BAD_VIDEO)
    total = video.size + audio_packets(n_frames, frame_bytes, frames_per_pes) * 188
    if dst_stride is not None and total > dst_stride:
        return (b"", MUX_FULL, []) if want_units else (b"", MUX_FULL)
    audio = []
    for j in range(0, n_frames, frames_per_pes):
        payload = frames[j * frame_bytes:min(n_frames, j + frames_per_pes) * frame_bytes].tobytes()
        p = audio_pts(first_frame + j, first_pts, spf, rate)
        pes = b"\x00\x00\x01\xC0" + (8 + len(payload)).to_bytes(2, "big") + b"\x80\x80\x05" + pts_bytes(p) + payload
        pk = packets(pes, pid, cc)
        cc = (cc + len(pk) // 188) & 15
        audio.append((p, pk))
    out, order = bytearray(), []
    ai, reach = 0, -1  # reach: the largest video PTS so far (a PES without PTS counts as having its predecessor's)
    for first, n, pts in units:
        if pts is not None:
            reach = max(reach, pts)
        while ai < len(audio) and audio[ai][0] <= reach:
            order.append(("a", audio[ai][0], len(out) // 188, len(audio[ai][1]) // 188))
            out += audio[ai][1]
            ai += 1
        order.append(("v", pts, len(out) // 188, n))
        out += video[first * 188:(first + n) * 188].tobytes()
    for p, pk in audio[ai:]:
        order.append(("a", p, len(out) // 188, len(pk) // 188))
        out += pk
    assert len(out) == total
    return (bytes(out), 0, order) if want_units else (bytes(out), 0)


def video_only(ts: np.ndarray) -> np.ndarray:
    """The PID-0x100 packets of a transport stream (the reference's clips also carry PAT, PMT and audio)."""
    pk = np.asarray(ts, dtype=np.uint8).reshape(-1, 188)
    pid = ((pk[:, 1].astype(np.int32) & 0x1F) << 8) | pk[:, 2]
    return pk[pid == 0x100].reshape(-1).copy()
