// k_mux.hip -- video transport stream + SBC frames -> one transport stream the reference player plays: efx_mux_av.
//
// The player takes video from PID 0x100 and audio from PES packets on PID 0x101 / 0x102 of the same stream
// (MpegDecoder::demux, reference src/player.cpp:381-493; audio: 421-433).  The unit of interleaving is a PES: the
// packets of one PES stay together, video packets are copied unchanged, the audio frames are wrapped in PES of
// frames_per_pes frames (00 00 01 C0, length, 80 80 05, PTS) and 188-byte packets the way k_enc_pack wraps video.
// Units appear in PTS order, audio first at equal PTS, the order inside each kind kept.
//
// ONE workgroup per stream, no unit list: with M[i] = the largest video PTS in packets 0 .. i (a PES without PTS adds
// nothing: it counts as its predecessor's) and A(t) = the audio PES with PTS <= t (their PTS are an arithmetic formula:
// a binary search, no table), a two-pointer merge puts
//     video packet i  at output packet  i + packets of the first A(M[i]) audio PES
//     audio PES j     at output packet  j x (packets of a full PES) + the first i with A(M[i]) > j   (all of them: at the end)
// so one prefix maximum over the packets, 256 at a time, places everything:
//   pass 0  every packet: sync byte, PID 0x100; the first starts a PES       -> EFX_MUX_BAD_VIDEO, nothing written
//   pass 1  per 256 packets: A of the PES starts, prefix maximum, the packets copied as dwords (a packet is 47 of them, and
//           188-byte steps keep source and destination 4-byte aligned, not 16), and where A steps up the audio PES that go
//           in front of packet i noted in video_before[]
//   pass 2  every dword of every audio packet synthesised from the frames.
#include <hip/hip_runtime.h>

#include "efx_internal.h"
#include "efx.h"
#include "enc_core.h"

namespace efx {

namespace {

constexpr int kMuxThreads = 256;
constexpr int kPesHdr = 14;  // 00 00 01 C0, length, 80 80 05, PTS

__device__ inline int64_t audio_pes_pts(const MuxArgs& a, int j)
{
    return a.first_pts + (a.first_frame + (int64_t)j * a.frames_per_pes) * a.samples_per_frame * 90000 / a.sample_rate;
}

// audio PES with PTS <= t
__device__ inline int audio_upto(const MuxArgs& a, int64_t t)
{
    int lo = 0, hi = a.n_pes;  // PES [0, lo) qualify, [hi, n) do not
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (audio_pes_pts(a, mid) <= t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// packets of the first k audio PES (only the last PES of a call can be short)
__device__ inline uint32_t audio_packets_of(const MuxArgs& a, int k) { return k >= a.n_pes ? (uint32_t)a.audio_packets : (uint32_t)k * a.pes_packets; }

// A video packet that starts a PES: its PTS, or -1 if the PES header carries none.  *ok: the payload begins 00 00 01.
__device__ inline int64_t video_start_pts(const uint8_t* p, bool* ok)
{
    const uint32_t afc = (p[3] >> 4) & 3;
    uint32_t off = 4;
    if (afc & 2)
        off += 1u + p[4];
    *ok = (afc & 1) && off + 9 <= 188 && p[off] == 0 && p[off + 1] == 0 && p[off + 2] == 1;
    if (!*ok || !(p[off + 7] & 0x80) || off + kPesHdr > 188)
        return -1;
    const uint8_t* t = p + off + 9;
    return ((int64_t)((t[0] >> 1) & 7) << 30) | ((int64_t)t[1] << 22) | ((int64_t)(t[2] >> 1) << 15) | ((int64_t)t[3] << 7) | (t[4] >> 1);
}

// byte o of the packets of audio PES j (n_fr frames), the first packet with continuity counter cc0
__device__ inline uint8_t audio_byte(const MuxArgs& a, const uint8_t* frames, int j, int n_fr, uint32_t cc0, uint32_t o)
{
    const uint32_t payload = (uint32_t)n_fr * a.frame_bytes;
    int64_t pp;
    uint8_t b = enc::ts_byte(o, payload + kPesHdr, cc0, &pp);
    const uint32_t in_pkt = o % 188;
    if (in_pkt == 1)
        b = (uint8_t)((b & 0x40) | (a.pid >> 8));
    else if (in_pkt == 2)
        b = (uint8_t)(a.pid & 0xFF);
    if (pp < 0)
        return b;
    if (pp >= kPesHdr)
        return frames[(size_t)j * a.frames_per_pes * a.frame_bytes + (size_t)(pp - kPesHdr)];
    switch ((int)pp) {
    case 3: return 0xC0;
    case 4: return (uint8_t)((8 + payload) >> 8);  // PES_packet_length: what follows it, 3 + 5 header bytes and the frames
    case 5: return (uint8_t)(8 + payload);
    default: return enc::pes_header_byte((int)pp, audio_pes_pts(a, j) & ((1ll << 33) - 1));
    }
}

}  // namespace

// grid = streams, block = 256
__global__ __launch_bounds__(kMuxThreads) void k_mux(MuxArgs a)
{
    __shared__ uint32_t sh_bad;
    __shared__ int sh_scan[kMuxThreads];
    __shared__ uint32_t sh_to[kMuxThreads];  // output packet of the chunk's packets
    __shared__ int sh_carry;

    const int s = blockIdx.x, tid = threadIdx.x;
    const uint32_t vlen = a.video_len[s];
    const uint32_t n_pkts = vlen / 188;
    const uint8_t* video = a.video + (size_t)s * a.video_stride;
    const uint8_t* frames = a.audio + (size_t)s * a.audio_stride;
    uint8_t* dst = a.dst + (size_t)s * a.dst_stride;
    uint32_t* video_before = a.video_before + (size_t)s * (a.n_pes > 0 ? a.n_pes : 1);
    const uint64_t total = ((uint64_t)n_pkts + (uint32_t)a.audio_packets) * 188;

    if (tid == 0) {
        sh_bad = (vlen % 188) ? EFX_MUX_BAD_VIDEO : 0u;
        sh_carry = 0;
    }
    __syncthreads();
    // ---- pass 0: is it a video transport stream? ---------------------------------------------------------------
    if (!sh_bad) {
        bool bad = false;
        for (uint32_t i = tid; i < n_pkts; i += kMuxThreads) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(video + (size_t)i * 188);  // 47 xx xx xx, little endian
            bad |= (w & 0xFF) != 0x47 || ((w >> 8) & 0x1F) != 0x01 || ((w >> 16) & 0xFF) != 0x00;
            if (i == 0) {
                bool ok;
                (void)video_start_pts(video, &ok);
                bad |= !(w & 0x4000) || !ok;
            }
        }
        if (bad)
            sh_bad = EFX_MUX_BAD_VIDEO;  // (plain stores of one value)
    }
    __syncthreads();
    uint32_t st = sh_bad;
    if (!st && total > a.dst_stride)
        st = EFX_MUX_FULL;
    if (st) {
        if (tid == 0) {
            a.len[s] = 0;
            a.status[s] = st;
        }
        return;
    }
    for (int j = tid; j < a.n_pes; j += kMuxThreads)
        video_before[j] = n_pkts;  // (audio later than the last video PES follows it)
    __syncthreads();

    // ---- pass 1: place and copy the video packets ----------------------------------------------------------------
    for (uint32_t i0 = 0; i0 < n_pkts; i0 += kMuxThreads) {
        const uint32_t i = i0 + tid;
        int mine = 0;
        if (i < n_pkts) {
            const uint8_t* p = video + (size_t)i * 188;
            if (p[1] & 0x40) {
                bool ok;
                const int64_t pts = video_start_pts(p, &ok);
                if (pts >= 0)
                    mine = audio_upto(a, pts);
            }
        }
        // inclusive prefix maximum over the chunk, the chunks before it in sh_carry
        sh_scan[tid] = mine;
        __syncthreads();
        for (int d = 1; d < kMuxThreads; d <<= 1) {
            const int other = tid >= d ? sh_scan[tid - d] : 0;
            __syncthreads();
            sh_scan[tid] = max(sh_scan[tid], other);
            __syncthreads();
        }
        const int carry = sh_carry;
        const int incl = max(sh_scan[tid], carry), excl = tid ? max(sh_scan[tid - 1], carry) : carry;
        if (i < n_pkts) {
            sh_to[tid] = i + audio_packets_of(a, incl);
            for (int j = excl; j < incl; j++)
                video_before[j] = i;
        }
        __syncthreads();
        if (tid == kMuxThreads - 1)
            sh_carry = incl;
        const uint32_t n_here = min((uint32_t)kMuxThreads, n_pkts - i0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(video + (size_t)i0 * 188);
        for (uint32_t d = tid; d < n_here * 47; d += kMuxThreads) {
            const uint32_t k = d / 47, w = d - k * 47;
            reinterpret_cast<uint32_t*>(dst + (size_t)sh_to[k] * 188)[w] = src[d];
        }
        __syncthreads();
    }

    // ---- pass 2: the audio packets ---------------------------------------------------------------------------------
    // (video_before[] was written by this workgroup: the barriers above make it visible)
    const uint32_t n_words = (uint32_t)a.audio_packets * 47;
    for (uint32_t d = tid; d < n_words; d += kMuxThreads) {
        const uint32_t ap = d / 47, w = d - ap * 47;                    // audio packet of the stream, dword of it
        const int j = min((int)(ap / (uint32_t)a.pes_packets), a.n_pes - 1);
        const uint32_t pk = ap - (uint32_t)j * a.pes_packets;            // packet of the PES
        const int n_fr = min(a.frames_per_pes, a.n_frames - j * a.frames_per_pes);
        const uint32_t cc0 = ((uint32_t)a.cc + (uint32_t)j * a.pes_packets) & 15;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            v |= (uint32_t)audio_byte(a, frames, j, n_fr, cc0, pk * 188 + w * 4 + b) << (8 * b);
        reinterpret_cast<uint32_t*>(dst + ((size_t)video_before[j] + ap) * 188)[w] = v;
    }
    if (tid == 0) {
        a.len[s] = (uint32_t)total;
        a.status[s] = 0;
    }
}

}  // namespace efx
