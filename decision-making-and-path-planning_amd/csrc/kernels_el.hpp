// kernels_el.hpp — episode log (build-defined): k_log_episodes appends one EpisodeRecord per episode that the advance
// ended to a ring on the device.  It runs on the upload stream directly behind k_respawn_egos / k_respawn_spawn - which it leaves as
// they are: it reads what they left behind - in front of the traffic kernels, and is launched only while the log is on.
//
// ONE workgroup of sixteen waves strides the scenes in chunks of its own size, 1024 - the kernel sits in the serial chain of an
// advance, and a chunk is a round trip to memory and a barrier -: ended scenes are few per advance and the scan reads one word per
// scene.  The order of the records - by advance, then by scene index - is part of the specification, so a record's slot
// comes from a scan, never from who gets to a counter first: per chunk one ballot per wave (ended scenes below a lane: a popcount
// of the ballot under the lane's mask), the sixteen wave totals exchanged through LDS (two sets, used in turn: one barrier per chunk)
// and a running base carried over the chunks.  A launch that ends more episodes than the ring holds drops its own oldest records, so a
// first pass counts the ended scenes the same way.  `total` is read by every thread in front of the first barrier and written by one
// thread behind the last; stream order serialises the launches.  No scratch, 128 B of LDS.
#pragma once
#include "kernels_sc.hpp"

namespace dmpp {

static_assert(sizeof(EpisodeRecord) == 240 && offsetof(EpisodeRecord, scene) == 0 && offsetof(EpisodeRecord, episode) == 4 && offsetof(EpisodeRecord, start) == 8 &&
              offsetof(EpisodeRecord, cause) == 12 && offsetof(EpisodeRecord, age) == 16 && offsetof(EpisodeRecord, seq) == 20 && offsetof(EpisodeRecord, tick) == 24 &&
              offsetof(EpisodeRecord, dist) == 32 && offsetof(EpisodeRecord, end_pos) == 40 && offsetof(EpisodeRecord, end_speed) == 56 &&
              offsetof(EpisodeRecord, score) == 64, "EpisodeRecord layout (DESIGN.md §4n)");
static_assert(sizeof(EpisodeRecord) % 16 == 0 && sizeof(RolloutScore) == 176 && offsetof(EpisodeRecord, score) % 16 == 0, "a record is fifteen 16-byte pieces, the last eleven its scorecard");
typedef unsigned int RecordPiece __attribute__((ext_vector_type(4)));      // (a native vector: one 16-byte store, which the compiler does not take apart)
struct RecordPieces { RecordPiece p[15]; };
static_assert(sizeof(RecordPieces) == sizeof(EpisodeRecord), "the pieces of a record");
constexpr int kLogBlock = 1024, kLogWaves = kLogBlock / DMPP_WAVE;      // the largest workgroup: 16 waves, 4 per SIMD of one CU (<= 128 VGPRs each)

// the ended scenes of chunk `base` in the waves below `wave`, and in the whole chunk: every wave's count goes through LDS set `set`
__device__ __forceinline__ void chunk_counts(int (&cnt)[2][kLogWaves], int set, int wave, int lane, int mine, int& below, int& all)
{
    if (lane == 0) cnt[set][wave] = mine;
    __syncthreads();
    below = 0; all = 0;
#pragma unroll
    for (int w = 0; w < kLogWaves; w++) { const int c = cnt[set][w]; if (w < wave) below += c; all += c; }
}

// prev: the SceneIn records the advance read; stats: EpisodeStats behind the episode step; sstats: EpisodeSpawnStats behind it, or null
// without a spawn model; ring[cap], total, start_of, ep_score: the log (ep_score null while the handle has no scorecard).
__global__ void __launch_bounds__(kLogBlock)
k_log_episodes(int n_scenes, int cap, int seq, long long tick, const SceneIn* __restrict__ prev, const EpisodeStats* __restrict__ stats,
               const EpisodeSpawnStats* __restrict__ sstats, EpisodeRecord* __restrict__ ring, long long* __restrict__ total,
               int32_t* __restrict__ start_of, RolloutScore* __restrict__ ep_score)
{
    __shared__ int cnt[2][kLogWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (n_scenes <= 0 || cap <= 0) return;
    const long long t0 = *total;
    // m, the ended scenes of the launch: the records from ordinal t0 + m - cap on are kept
    int wave_m = 0;                                      // ... of this wave's lanes, over all chunks
    for (int base = 0; base < n_scenes; base += kLogBlock) {
        const int s = base + tid;
        wave_m += __popcll(wave_ballot(s < n_scenes && stats[s].age == 0));
    }
    int unused, m;
    chunk_counts(cnt, 0, wave, lane, wave_m, unused, m);
    const long long first = t0 + (long long)m - (long long)cap;
    __syncthreads();                                     // set 0 is written again by the first chunk below
    long long o = t0;                                    // ordinal of the first ended scene of the chunk
    int set = 0;
    for (int base = 0; base < n_scenes && o < t0 + m; base += kLogBlock, set ^= 1) {
        const int s = base + tid;
        const bool ended = s < n_scenes && stats[s].age == 0;
        const unsigned long long b = wave_ballot(ended);
        int below, all;
        chunk_counts(cnt, set, wave, lane, __popcll(b), below, all);
        if (ended) {
            const long long ord = o + below + __popcll(b & ((1ull << lane) - 1ull));
            const EpisodeStats& e = stats[s];
            const RolloutScore sc = ep_score ? ep_score[s] : score_start();
            if (ord >= first) {
                const LocationOut& L = prev[s].loc;
                EpisodeRecord r;
                r.scene = s; r.episode = e.n_episodes - 1; r.start = start_of[s]; r.cause = e.last_cause;
                r.age = e.last_age; r.seq = seq; r.tick = tick; r.dist = e.last_dist;
                r.end_pos.x = L.globalpoint.x; r.end_pos.y = L.globalpoint.y; r.end_speed = L.velocity;
                r.score = sc;
                // 240 B divide into fifteen 16-byte pieces, and a device allocation starts on a 16-byte boundary: so does every record
                const RecordPieces q = __builtin_bit_cast(RecordPieces, r);
                RecordPiece* dst = reinterpret_cast<RecordPiece*>(ring + (size_t)(ord % (long long)cap));
#pragma unroll
                for (int i = 0; i < 15; i++) dst[i] = q.p[i];
            }
            if (ep_score) ep_score[s] = score_start();
            start_of[s] = sstats ? sstats[s].cur_start : 0;
        }
        o += all;
    }
    if (tid == 0) *total = t0 + m;
}

}  // namespace dmpp
