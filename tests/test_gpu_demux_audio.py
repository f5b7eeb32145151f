"""efx_demux_audio across its chunks of 16 packets and its rounds of 64 chunks: the gate of player.cpp:421-433 (audio
bytes count only while the latest audio PES start carried a PTS) and the bytes pending under it, carried from chunk to
chunk and from round to round (k_demux_audio_scan / _offsets / k_demux_audio), against the oracle."""
import numpy as np
import pytest

import common
import oracle

pytestmark = pytest.mark.gpu

# kept of offered audio payload bytes, as the oracle, the reference player and a model of the three kernels agree
KEPT = {"late_open": (4301, 86857), "long_open_long_closed": (157484, 237424), "boundaries": (71330, 74433),
        "hostile_long": (92105, 121117)}


def test_gates_across_chunks_and_rounds():
    import espflix_amd as efx
    efx.load_library()
    cases = {**common.audio_gate_streams(), **common.audio_gate_cut_streams()}
    whole = cases["late_open"]
    cases.update({"empty": b"", "p16": whole[:16 * 188], "p17": whole[:17 * 188]})
    names, streams = list(cases), list(cases.values())
    assert [len(cases[f"exact{n}"]) // 188 for n in (1024, 1025, 1040)] == [1024, 1025, 1040]
    assert min(len(cases[n]) // 188 for n in KEPT) > 1024 and len(cases["hostile_long"]) // 188 > 2000
    stride = (max(len(s) for s in streams) + 255) & ~255
    dec = efx.Decoder(len(streams), 1, 2, max_stream_bytes=sum(len(s) for s in streams) + 16 * len(streams) + 4096)
    d_audio, d_len = dec.alloc(len(streams) * stride), dec.alloc(len(streams) * 4)
    dec.demux_audio(streams, d_audio, stride, d_len)
    lens = d_len.download(np.uint32, len(streams))
    audio = d_audio.download(np.uint8, len(streams) * stride).reshape(len(streams), stride)
    dec.close()
    for i, (name, ts) in enumerate(zip(names, streams)):
        want = oracle.ts_audio_es(np.frombuffer(ts, dtype=np.uint8))
        offered = common.audio_payload_offered(ts)
        print(name, len(ts) // 188, "packets: kept", int(lens[i]), "oracle", want.size, "offered", offered)
        assert lens[i] == want.size, (name, int(lens[i]), want.size)
        assert np.array_equal(audio[i, :lens[i]], want), name
        if name in KEPT:
            assert (want.size, offered) == KEPT[name], name
        if name in KEPT or name.startswith("exact"):
            assert 0 < want.size < offered, name   # a kept and a dropped stretch are both there
    assert lens[names.index("empty")] == 0
