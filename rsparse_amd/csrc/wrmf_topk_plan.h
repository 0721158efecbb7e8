// The launch plan of the top-k product (wrmf_topk.hip), computed once per call on the host: how the call is sliced, where the
// candidate buffers live, how much scratch it wants, and every launch of a product kernel in order with its geometry.  Whoever
// needs to know which kernel will run -- the C ABI sizing its scratch, launch_top_product{,_f64} walking the launches,
// rsparse_hip_top_product_plan reporting them -- reads this plan.  Plain C++: no HIP type, no device call.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#ifdef __HIPCC__
#define RSP_TOPK_HD __host__ __device__
#else
#define RSP_TOPK_HD
#endif

namespace rsparse_hip {

constexpr int kTopBlock = 32;    // users per MFMA block
constexpr int kTopMaxK = 256;    // RSPARSE_HIP_MAX_TOPK
constexpr int kTopMaxCap = 576;  // no candidate buffer is longer (top_gcap(256) = 544; the LDS geometries: k + 128 at most)
constexpr size_t kTopLdsMax = 156 * 1024;
// candidate buffer per user: the heap (k entries) + everything one round can add (32 items per tile of the round)
RSP_TOPK_HD constexpr int top_cap(int topk, int tiles_per_round) { return ((topk + 32 * tiles_per_round + 3) / 4) * 4; }

// GBUF (round 6): the candidate buffers of 256 users fit the LDS next to two tiles only up to k = 27 at rank 128, and only without
// a spare entry: a user was settled at EVERY arrival.  The tile-sharing kernel now keeps them in GLOBAL memory (a scratch slot
// per workgroup: appends are fire-and-forget stores, only the counts and thresholds stay in LDS) with room for a BATCH of
// arrivals beyond one tile's worth -- a user is settled once per max(64, k) arrivals, in the settling wave's LDS work area,
// by a radix select (topk_reduce_user).  One geometry, 256 users per workgroup, for every k.
RSP_TOPK_HD constexpr int top_gcap(int topk) { return ((topk + 32 + (topk > 64 ? topk : 64) + 3) / 4) * 4; }
constexpr int kTopGbufChunk = 131072;   // users per launch of a GBUF call: 512 slots of scratch, two full rounds of workgroups

enum TopFamily { kTopPerWave, kTopShared, kTopPipe };   // top_product_kernel / _shared_kernel / _pipe_kernel
struct TopGeo {
  TopFamily family;
  int KP, UB, W;     // padded rank, 32-user blocks per wave (per workgroup in kTopPerWave), waves
  bool gbuf;         // candidate buffers in the global scratch
  int users, threads;
  size_t lds;
};
struct TopLaunch {
  TopGeo geo;
  int user0, n_users, topk, n_slices, slice_items, grid_x;
  bool flagged;      // a re-run: only the workgroups that hold a flagged user do anything
};
struct TopPlan {
  bool valid = false;
  int n_slices = 1, slice_items = 0;   // of the nominating pass (1 = unsliced)
  bool gbuf = false;                   // ... and whether it keeps its buffers in the scratch
  size_t scratch_floats = 0;           // what the call wants (0 = none)
  std::vector<TopLaunch> launches;     // the last one is the re-run at topk when the re-scoring pass follows
  int n_first = 0;                     // launches of the nominating pass (before that re-run)
};

inline int top_padded_rank(int k) { return k < 1 ? 0 : (k <= 32 ? 32 : (k <= 64 ? 64 : (k <= 128 ? 128 : (k <= 256 ? 256 : 0)))); }

// how a call is split: slices of `slice_items` items (a multiple of 32), 1 = not at all
inline int top_product_slices(int n_users, int n_items, int topk, int* slice_items) {
  *slice_items = 0;
  // (users per workgroup of the geometry the table below picks for this many users; a smaller one -- when the candidate
  //  buffers of a large k do not fit -- only means more workgroups than planned)
  const int upw = n_users > 128 ? 256 : (n_users > 64 ? 128 : (n_users > 32 ? 64 : 32));
  const int ublocks = (n_users + upw - 1) / upw;
  const int n_tiles = (n_items + 31) / 32;
  if (n_users <= 0 || ublocks >= 128 || n_tiles < 128) return 1;   // enough workgroups already, or nothing to split
  int S = std::min(64, std::min((512 + ublocks - 1) / ublocks, n_tiles / 32));
  if ((size_t)S * n_users * topk > ((size_t)8 << 20)) S = (int)(((size_t)8 << 20) / ((size_t)n_users * topk));
  if (S < 2) return 1;
  const int st = (n_tiles + S - 1) / S;
  *slice_items = 32 * st;
  return (n_tiles + st - 1) / st;
}

// LDS of a geometry: the item tiles (rows of KP + 4 floats), the candidate buffers (or, GBUF, per wave a work area and a scratch),
// counts / thresholds / verified lengths, per wave the compaction scratch
inline size_t top_lds_bytes(TopFamily family, int KP, int UB, int W, bool gbuf, int topk) {
  const size_t ldt = (size_t)KP + 4, users = (size_t)kTopBlock * UB * (family == kTopPerWave ? 1 : 4);
  if (family == kTopPerWave) {
    const size_t cap = (size_t)top_cap(topk, W);
    return ((size_t)W * 32 * ldt + 2 * users * cap + 8 * users) * 4 + 64 + (size_t)W * cap * 8;
  }
  const size_t tile_floats = (family == kTopPipe ? 2 : 1) * 32 * ldt, cap = (size_t)top_cap(topk, 1);
  if (gbuf) return (tile_floats + 3 * users) * 4 + 64 + (size_t)4 * top_gcap(topk) * 16;
  return (tile_floats + 2 * users * cap + 3 * users) * 4 + 64 + (size_t)4 * cap * 8;
}

// Geometry, best first: the four waves share the item tile and own 64 / 32 users each (256 / 128 users per workgroup: every item
// vector is read once per that many users) -- with two tiles resident and the epilogue hidden behind the next tile's matrix
// instructions where the LDS allows it; then one tile per wave against 64 / 32 users; then the same on two waves (half the tiles
// and half the per-round candidates in LDS: top-k up to 256 at rank 128).  What decides is whether the users' candidate buffers
// fit the LDS next to the tiles, and that there are users enough for the block.  The first row whose conditions hold wins; the
// last row of a rank has none.  (Rank 129..256: the user block of a wave is 128 registers, one block per wave in every geometry.)
// GBUF: every call for more than 128 users at a rank up to 128 that comes with a scratch: measured faster than the LDS buffers at
// EVERY k -- top-100 29 -> 86 TFLOP/s (the LDS took 32 users per workgroup there), top-10 80 -> 96, top-1 89 -> 98
// (profiles/r06/r6topk_*).  Rows that the LDS arithmetic can never select are not listed (profiles/topk_plan).
struct TopRow {
  TopFamily family;
  int UB, W;
  bool gbuf;
  int more_users_than, kp_min, kp_max;
};
constexpr TopRow kTopRows[] = {
    {kTopPipe, 2, 4, true, 128, 32, 128},   {kTopPipe, 2, 4, false, 128, 32, 128}, {kTopPipe, 1, 4, false, 64, 32, 256},
    {kTopShared, 1, 4, false, 64, 32, 256}, {kTopPerWave, 2, 4, false, 32, 32, 128}, {kTopPerWave, 1, 4, false, 0, 32, 128},
    {kTopPerWave, 1, 2, false, 0, 128, 256}};

inline bool top_product_wants_gbuf(int n_users, int k_rank, int topk) {
  return n_users > 128 && k_rank <= 128 && topk >= 1 && topk <= kTopMaxK && top_padded_rank(k_rank) != 0;
}

// one launch: `gbuf` = the launcher has a scratch for the candidate buffers (a flagged launch has at most 512 workgroups = scratch
// slots, whatever the number of users).  false: no kernel for this rank / k
inline bool top_plan_launch(TopLaunch* out, int user0, int n_users, int k_rank, int topk, int n_slices, int slice_items,
                            bool flagged, bool gbuf) {
  const int KP = top_padded_rank(k_rank);
  if (!KP || topk < 1 || topk > kTopMaxK) return false;
  const bool gbuf_now = gbuf && n_slices == 1 && (n_users <= kTopGbufChunk || flagged) && top_product_wants_gbuf(n_users, k_rank, topk);
  const TopRow* last = nullptr;
  for (const TopRow& r : kTopRows)
    if (KP >= r.kp_min && KP <= r.kp_max) last = &r;
  for (const TopRow& r : kTopRows) {
    if (KP < r.kp_min || KP > r.kp_max) continue;
    const size_t lds = top_lds_bytes(r.family, KP, r.UB, r.W, r.gbuf, topk);
    if (&r != last && !(r.gbuf ? gbuf_now : (lds <= kTopLdsMax && n_users > r.more_users_than))) continue;
    const int users = kTopBlock * r.UB * (r.family == kTopPerWave ? 1 : 4), blocks = (n_users + users - 1) / users;
    // (the two-tile kernel walks user blocks: a flagged launch is capped, see its block loop)
    const int grid_x = (r.family == kTopPipe && flagged) ? std::min(blocks, 512) : blocks;
    *out = TopLaunch{TopGeo{r.family, KP, r.UB, r.W, r.gbuf, users, 64 * r.W, lds}, user0, n_users, topk, n_slices, slice_items,
                     grid_x, flagged};
    return true;
  }
  return false;
}

// The whole call: n_users x n_items at `rank`; the nominating pass keeps kc per user (kc = topk: the fp32 form); `rescore`: the
// double re-scoring pass follows and, where kc > topk, the flagged re-run at topk; `scratch`: the caller brings the scratch this
// plan asks for (without one nothing is sliced and the buffers stay in LDS).
inline TopPlan top_product_plan(int n_users, int n_items, int rank, int kc, int topk, bool rescore, bool scratch = true) {
  TopPlan p;
  TopLaunch l;
  int slice_items = 0;
  const int S = scratch ? top_product_slices(n_users, n_items, kc, &slice_items) : 1;
  const bool gbuf = scratch && S <= 1 && top_product_wants_gbuf(n_users, rank, kc);
  if (!top_plan_launch(&l, 0, std::max(n_users, 1), rank, kc, 1, 0, false, false)) return p;   // (rank / k without a kernel)
  p.valid = true;
  if (n_users <= 0) return p;
  if (S > 1) {
    // few users, many items: the slices' lists land in the scratch (scores, indices, a flag per user) and are merged; users
    // whose merged list is ambiguous are recomputed by the unsplit kernel
    p.n_slices = S;
    p.slice_items = slice_items;
    p.scratch_floats = 2 * (size_t)S * n_users * kc + (size_t)n_users + 16;
    top_plan_launch(&l, 0, n_users, rank, kc, S, slice_items, false, false);
    p.launches.push_back(l);
    top_plan_launch(&l, 0, n_users, rank, kc, 1, 0, true, false);
    p.launches.push_back(l);
  } else if (gbuf) {
    // the candidate buffers in the scratch: chunks of users, one after the other on the stream, share its 512 slots
    p.gbuf = true;
    p.scratch_floats = (((size_t)std::min(n_users, kTopGbufChunk) + 255) / 256) * 2 * 256 * (size_t)top_gcap(kc) + 16;
    for (int c0 = 0; c0 < n_users; c0 += kTopGbufChunk) {
      top_plan_launch(&l, c0, std::min(kTopGbufChunk, n_users - c0), rank, kc, 1, 0, false, true);
      p.launches.push_back(l);
    }
  } else {
    top_plan_launch(&l, 0, n_users, rank, kc, 1, 0, false, false);
    p.launches.push_back(l);
  }
  p.n_first = (int)p.launches.size();
  if (rescore && kc > topk) {
    // (the tile-sharing kernel with its block loop and the global buffers where the scratch was sized for them -- an unsliced call
    //  for more than 128 users --, else the geometry the LDS allows)
    if (!top_plan_launch(&l, 0, n_users, rank, topk, 1, 0, true, scratch && S <= 1 && top_product_wants_gbuf(n_users, rank, topk)))
      p.valid = false;
    p.launches.push_back(l);
  }
  return p;
}

}  // namespace rsparse_hip
