// cutfemx_amd: level-set classification, selector scan, cell neighbours, ghost-penalty / interior / exterior
// facet selection, facet hosts and cell aggregation -- HIP kernels for gfx950 and their C ABI.  What is built on a
// classified cut -- sub-triangulation, runtime quadrature, per-point evaluators -- is cfx_rules.hip.
//
// Replaces (paths relative to the CutFEMx tree):
//   cpp/cutfemx/cut/cut.cpp:845-868   update()  -> cutcells::cut        (a1)
//   cpp/cutfemx/cut/cut.cpp:877-924   locate_entities()                  (a4)
//   python/cutfemx/cut.py:340-380     ghost_penalty_facets()             (a7)
#include <cctype>
#include <cstdlib>
#include <cstring>

#include "cfx_cut.h"
#include "cfx_device.h"

using namespace cfx;

namespace cfx
{
Selector parse_selector(const char* s, int nls)
{
  require(s != nullptr, CFX_ERR_INVALID_ARGUMENT, "selector is null");
  Selector sel;
  int term = 0;
  const char* p = s;
  auto fail = [&](const char* why)
  { throw Error(CFX_ERR_INVALID_ARGUMENT, std::string("invalid selector '") + s + "': " + why); };
  for (;;)
  {
    while (*p && isspace((unsigned char)*p)) ++p;
    if (!*p) fail("expected a level-set name");
    const char* b = p;
    while (*p && (isalnum((unsigned char)*p) || *p == '_')) ++p;
    if (p == b) fail("expected a level-set name");
    const size_t len = (size_t)(p - b);
    int ls = -1;
    if (len >= 3 && strncmp(b, "phi", 3) == 0)
    {
      ls = 0;
      for (size_t i = 3; i < len; ++i)
      {
        if (!isdigit((unsigned char)b[i])) { ls = -1; break; }
        ls = 10 * ls + (b[i] - '0');
      }
    }
    if (ls < 0 || ls >= nls) fail("unknown level-set name");
    while (*p && isspace((unsigned char)*p)) ++p;
    int mask = 0;
    if (p[0] == '<' && p[1] == '=') { mask = 1 | 2; p += 2; }
    else if (p[0] == '>' && p[1] == '=') { mask = 4 | 2; p += 2; }
    else if (p[0] == '=' && p[1] == '=') { mask = 2; p += 2; }
    else if (p[0] == '<') { mask = 1; p += 1; }
    else if (p[0] == '>') { mask = 4; p += 1; }
    else if (p[0] == '=') { mask = 2; p += 1; }
    else fail("expected a relation (<, <=, =, >=, >)");
    while (*p && isspace((unsigned char)*p)) ++p;
    char* e = nullptr;
    const double rhs = strtod(p, &e);
    if (e == p || rhs != 0.0) fail("right-hand side must be 0");
    p = e;
    if (sel.n >= kMaxClauses) fail("too many clauses");
    sel.ls[sel.n] = ls; sel.mask[sel.n] = mask; sel.term[sel.n] = term; ++sel.n;
    while (*p && isspace((unsigned char)*p)) ++p;
    if (!*p) break;
    if (strncmp(p, "and", 3) == 0) p += 3;
    else if (strncmp(p, "&&", 2) == 0) p += 2;
    else if (*p == '&') p += 1;
    else if (strncmp(p, "or", 2) == 0) { p += 2; ++term; }
    else if (strncmp(p, "||", 2) == 0) { p += 2; ++term; }
    else if (*p == '|') { p += 1; ++term; }
    else fail("expected 'and' / 'or'");
  }
  return sel;
}
} // namespace cfx

namespace
{

// ---------------------------------------------------------------------------
// a1 classification: one thread per cell, coalesced dofmap rows (16 B/lane for
// tets), gathered level-set values (L2/MALL resident), 1 B/cell out.
// ---------------------------------------------------------------------------
// sign code of every level-set dof: 1 negative, 2 positive, 0 zero.  The bitwise AND of a cell's
// codes is 1 iff all its values are negative, 2 iff all are positive, 0 otherwise -- and the byte
// table (135 MB at 512^3) stays in the Infinity Cache where the 1.1 GB of doubles does not.
// (zero_n > 0: the first zero_n threads also clear the per-tile counters of the classification that follows -- a fill
// launch less per step)
// (touch, optional: one byte per level-set dof, cleared here and set by the classification on the dofs of every cut cell)
__global__ void __launch_bounds__(kBlock) sign_codes_kernel(int64_t n, const double* __restrict__ phi, uint8_t* __restrict__ code,
                                                            int32_t* __restrict__ zero_this, int64_t zero_n,
                                                            uint8_t* __restrict__ touch)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < zero_n) zero_this[i] = 0;
  if (i >= n) return;
  const double v = phi[i];
  code[i] = v < 0.0 ? (uint8_t)1 : (v > 0.0 ? (uint8_t)2 : (uint8_t)0);
  if (touch) touch[i] = 0;
}

// the same, four values per thread: two 16 B loads and one 4 B store per lane (a byte per lane and store reached
// 4.1 TB/s of the level set at 512^3).  phi and code start on 16 B / 4 B boundaries (checked at the launch); the last
// n % 4 values go to the last thread one by one.
__global__ void __launch_bounds__(kBlock) sign_codes4_kernel(int64_t n, const double* __restrict__ phi, uint8_t* __restrict__ code,
                                                             int32_t* __restrict__ zero_this, int64_t zero_n,
                                                             uint8_t* __restrict__ touch)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < zero_n) zero_this[i] = 0;
  const int64_t b = 4 * i;
  if (b >= n) return;
  auto sign = [](double v) { return v < 0.0 ? 1u : (v > 0.0 ? 2u : 0u); };
  if (b + 4 <= n)
  {
    const double2 p = *reinterpret_cast<const double2*>(phi + b), q = *reinterpret_cast<const double2*>(phi + b + 2);
    *reinterpret_cast<uint32_t*>(code + b) = sign(p.x) | (sign(p.y) << 8) | (sign(q.x) << 16) | (sign(q.y) << 24);
    if (touch) *reinterpret_cast<uint32_t*>(touch + b) = 0u; // (as aligned as the codes: checked at the launch)
    return;
  }
  for (int64_t k = b; k < n; ++k)
  {
    code[k] = (uint8_t)sign(phi[k]);
    if (touch) touch[k] = 0;
  }
}

#ifndef CFX_CLASSIFY_UNROLL
#define CFX_CLASSIFY_UNROLL 4
#endif
template <int ND>
__global__ void __launch_bounds__(kBlock) classify_kernel(int64_t ncells, const int32_t* __restrict__ dofmap,
                                                          const uint8_t* __restrict__ code, int8_t* __restrict__ domain,
                                                          int32_t* tiles_inside, int32_t* tiles_cut,
                                                          uint8_t* __restrict__ touch = nullptr)
{
  // U cells per thread, a block-wide stride apart: U independent 16 B/lane streaming loads in
  // flight per lane before the first dependent level-set gather
  constexpr int U = CFX_CLASSIFY_UNROLL;
  const int64_t c0 = (int64_t)blockIdx.x * (kBlock * U) + threadIdx.x;
  int32_t d[U][ND];
  int n_in = 0, n_cut = 0;
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    const int64_t c = c0 + (int64_t)u * kBlock;
    if (c >= ncells) continue;
    if constexpr (ND == 4)
    {
      typedef int cfx_i4 __attribute__((ext_vector_type(4)));
      const cfx_i4 v = __builtin_nontemporal_load(reinterpret_cast<const cfx_i4*>(dofmap + c * 4)); // streamed once
      d[u][0] = v.x; d[u][1] = v.y; d[u][2] = v.z; d[u][3] = v.w;
    }
    else
    {
#pragma unroll
      for (int i = 0; i < ND; ++i) d[u][i] = dofmap[c * ND + i];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    const int64_t c = c0 + (int64_t)u * kBlock;
    if (c >= ncells) continue;
    unsigned all = 3u;
#pragma unroll
    for (int i = 0; i < ND; ++i) all &= code[d[u][i]];
    domain[c] = all == 1u ? (int8_t)CFX_INSIDE : (all == 2u ? (int8_t)CFX_OUTSIDE : (int8_t)CFX_INTERSECTED);
    n_in += all == 1u ? 1 : 0;
    n_cut += (all != 1u && all != 2u) ? 1 : 0;
    if (touch && all != 1u && all != 2u) // (a cut cell: its dofs are next to the interface; every writer stores 1)
    {
#pragma unroll
      for (int i = 0; i < ND; ++i) touch[d[u][i]] = 1;
    }
  }
  // the two selector scans every solve starts with ("phi<0", "phi=0") get their tile counts here
  if (tiles_inside)
  {
    static_assert(kByteTile % (kBlock * U) == 0, "classification blocks must nest in compaction tiles");
    int tot_in, tot_cut;
    (void)block_exclusive_scan<int>(n_in, tot_in);
    (void)block_exclusive_scan<int>(n_cut, tot_cut);
    if (threadIdx.x == 0)
    {
      const int64_t tile = ((int64_t)blockIdx.x * (kBlock * U)) / kByteTile;
      if (tot_in) atomicAdd(&tiles_inside[tile], tot_in);
      if (tot_cut) atomicAdd(&tiles_cut[tile], tot_cut);
    }
  }
}

// ---------------------------------------------------------------------------
// Classification with block culling.  The reference classifies cell by cell (cut.cpp:743-786); so did rounds 1-3,
// streaming the 16 B connectivity row of every one of the 805 M cells of the 512^3 mesh -- 12.9 GB, 2.8 ms, for a
// domain whose interface touches 0.35 % of the cells.  A block of kClassBlock consecutive cells whose vertices ALL have
// negative (all positive) level-set values consists of inside (outside) cells: that is decided from the block's
// mesh-static vertex summary (cfx_mesh_s::class_runs: the distinct vertices as runs of consecutive ids -- 4 to 12 runs on
// meshes whose numbering has any locality, ~0.7 KB of sign codes per block read coalesced) and written as one 1 KB
// run of the domain array; only blocks with vertices on both sides (or on the interface) read their connectivity and
// go cell by cell as before.  Same domain array bit for bit, any mesh; a block without a summary (more than kClassRuns
// runs: no locality in the numbering) always takes the cell-by-cell path.
// ---------------------------------------------------------------------------
template <int ND, int CELLS, int RUNS, int N, int H>
__global__ void __launch_bounds__(kBlock) class_summary_kernel(int64_t ncells, const int32_t* __restrict__ conn,
                                                               int32_t* __restrict__ nruns, int2* __restrict__ runs,
                                                               int2* __restrict__ sub_runs)
{
  constexpr int kClassBlock = CELLS, kClassRuns = RUNS; // (this kernel's block: the block proper, or a quarter of it)
  // the block's ND * kClassBlock vertex ids -> distinct ids (LDS hash set: a block of a mesh with any locality has a
  // few hundred) -> sorted (bitonic over N slots) -> runs of consecutive ids.  More than N distinct ids: no summary.
  constexpr int Q = N / kBlock;
  static_assert(N % kBlock == 0 && (H & (H - 1)) == 0 && H >= ND * CELLS, "summary table sizes");
  __shared__ int32_t s_h[H];
  __shared__ int32_t s_v[N];
  __shared__ int32_t s_start[kClassRuns + 1], s_d0[kClassRuns + 1];
  __shared__ int s_cnt;
  const int64_t c0 = (int64_t)blockIdx.x * kClassBlock;
  const int nloc = (int)(ncells - c0 < kClassBlock ? ncells - c0 : kClassBlock) * ND;
  for (int i = threadIdx.x; i < H; i += kBlock) s_h[i] = -1;
  for (int i = threadIdx.x; i < N; i += kBlock) s_v[i] = 0x7fffffff;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < nloc; i += kBlock)
  {
    const int32_t v = conn[c0 * ND + i];
    unsigned h = cfx_hash32((uint32_t)v) & (H - 1);
    for (int probe = 0; probe < H; ++probe)
    {
      const int32_t old = s_h[h];
      if (old == v) break;
      if (old == -1)
      {
        const int32_t prev = atomicCAS(&s_h[h], -1, v);
        if (prev == -1)
        {
          const int k = atomicAdd(&s_cnt, 1);
          if (k < N) s_v[k] = v;
          break;
        }
        if (prev == v) break;
      }
      h = (h + 1) & (H - 1);
    }
  }
  __syncthreads();
  const int ndist = s_cnt;
  if (ndist > N)
  {
    if (threadIdx.x == 0 && nruns) nruns[blockIdx.x] = -1;
    if (threadIdx.x < kClassRuns) runs[(int64_t)blockIdx.x * kClassRuns + threadIdx.x] = make_int2(0, threadIdx.x == 0 ? -1 : 0);
    if (sub_runs && threadIdx.x < kClassSub * kClassSubRuns)
      sub_runs[(int64_t)blockIdx.x * kClassSub * kClassSubRuns + threadIdx.x] = make_int2(0, threadIdx.x % kClassSubRuns == 0 ? -1 : 0);
    return;
  }
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
    {
      for (int i = threadIdx.x; i < N; i += kBlock)
      {
        const int p = i ^ j;
        if (p > i)
        {
          const int32_t a = s_v[i], b = s_v[p];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { s_v[i] = b; s_v[p] = a; }
        }
      }
      __syncthreads();
    }
  // the run starts among the (distinct, ascending) ids
  int isstart[Q], cs = 0;
#pragma unroll
  for (int q = 0; q < Q; ++q)
  {
    const int i = threadIdx.x * Q + q;
    isstart[q] = (i < ndist && (i == 0 || s_v[i - 1] != s_v[i] - 1)) ? 1 : 0;
    cs += isstart[q];
  }
  int tot_s;
  int os = block_exclusive_scan<int>(cs, tot_s);
  if (tot_s <= kClassRuns)
  {
#pragma unroll
    for (int q = 0; q < Q; ++q)
    {
      const int i = threadIdx.x * Q + q;
      if (isstart[q]) { s_start[os] = s_v[i]; s_d0[os] = i; ++os; }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && nruns) nruns[blockIdx.x] = tot_s <= kClassRuns ? tot_s : -1;
  // every slot is written: unused ones hold length 0, a block without a summary length -1 in slot 0 (the classification
  // reads the slots alone -- one dependent load less per wavefront)
  if (threadIdx.x < kClassRuns)
  {
    const int j = threadIdx.x;
    int2 r = make_int2(0, 0);
    if (tot_s > kClassRuns) r.y = j == 0 ? -1 : 0;
    else if (j < tot_s) r = make_int2(s_start[j], (j + 1 < tot_s ? s_d0[j + 1] : ndist) - s_d0[j]);
    runs[(int64_t)blockIdx.x * kClassRuns + j] = r;
  }
  if (sub_runs == nullptr) return;
  // The quarter blocks: per run of the block the span [min, max] of the ids the quarter's cells refer to -- a superset of
  // the quarter's vertices when they do not fill the span, which keeps the culling exact (one sign on a superset is one
  // sign on the set) and costs a search and two LDS atomics per reference where a summary of its own cost a hash set
  // and a sort per quarter (36 ms at 512^3).  Quarters that touch more than kClassSubRuns runs get no summary.
  __shared__ int32_t s_lo[kClassSub][RUNS], s_hi[kClassSub][RUNS];
  const bool have = tot_s <= kClassRuns;
  for (int i = threadIdx.x; i < kClassSub * RUNS; i += kBlock) { (&s_lo[0][0])[i] = 0x7fffffff; (&s_hi[0][0])[i] = -1; }
  __syncthreads();
  if (have)
    for (int i = threadIdx.x; i < nloc; i += kBlock)
    {
      const int32_t v = conn[c0 * ND + i];
      const int sq = (i / ND) / (CELLS / kClassSub);
      int lo = 0, hi = tot_s; // last run whose start is <= v
      while (hi - lo > 1)
      {
        const int mid = (lo + hi) >> 1;
        if (s_start[mid] <= v) lo = mid; else hi = mid;
      }
      atomicMin(&s_lo[sq][lo], v);
      atomicMax(&s_hi[sq][lo], v);
    }
  __syncthreads();
  if (threadIdx.x < kClassSub)
  {
    const int sq = threadIdx.x;
    int2* out = sub_runs + ((int64_t)blockIdx.x * kClassSub + sq) * kClassSubRuns;
    int n = 0;
    bool ok = have;
    for (int j = 0; ok && j < tot_s; ++j)
      if (s_hi[sq][j] >= 0)
      {
        if (n == kClassSubRuns) { ok = false; break; }
        out[n++] = make_int2(s_lo[sq][j], s_hi[sq][j] - s_lo[sq][j] + 1);
      }
    if (!ok) { n = 0; out[n++] = make_int2(0, -1); }
    for (; n < kClassSubRuns; ++n) out[n] = make_int2(0, 0);
  }
}

// The chunk descriptors of a block (cfx_mesh_s::class_chunks) from its runs, one wavefront per block: the aligned 16 B
// words of a sign-code array that the runs touch, ascending, each with the mask of its bytes that belong to a run.  The
// runs ascend and are at least one id apart, so a word is shared by neighbouring runs only: run j opens the words from
// its first to its last, less the first when run j - 1 ended in it (several short runs may lie in one word).  More than
// kClassChunks words, or no summary: -1 in the mask of slot 0.  Blocks from nblocks on (the padding to an even number)
// get empty descriptors.
__global__ void __launch_bounds__(kBlock) class_chunks_kernel(int64_t nblocks, int64_t nblocks_padded, const int2* __restrict__ runs,
                                                              int2* __restrict__ chunks)
{
  static_assert(kClassChunks == 64 && kClassRuns <= 64, "one descriptor and at most one run per lane");
  __shared__ int32_t s_word[kBlock / 64][kClassChunks];
  __shared__ uint32_t s_mask[kBlock / 64][kClassChunks];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (kBlock / 64) + w;
  const bool real = b < nblocks;
  int2 r = make_int2(0, 0);
  if (real && lane < kClassRuns) r = runs[b * kClassRuns + lane];
  const bool summary = real && __shfl(r.y, 0, 64) >= 0;
  const bool have = summary && r.y > 0;
  const int wlo = r.x >> 4, whi = (r.x + (have ? r.y - 1 : 0)) >> 4;
  const int prev_hi = __shfl_up(whi, 1, 64);
  const int first_new = wlo + ((have && lane > 0 && prev_hi == wlo) ? 1 : 0);
  const int cnt = have ? whi - first_new + 1 : 0;
  const int incl = wave_inclusive_scan<int>(cnt);
  const int total = __shfl(incl, 63, 64);
  const int off = incl - cnt;
  const bool fits = summary && total <= kClassChunks;
  s_word[w][lane] = 0; s_mask[w][lane] = 0u;
  __syncthreads();
  if (fits && have)
  {
    for (int k = 0; k < cnt; ++k) s_word[w][off + k] = first_new + k;
    for (int wd = wlo; wd <= whi; ++wd)
    {
      const int slot = off + (wd - first_new); // (off - 1: the word the run before ended in)
      const int lo = wd == wlo ? (r.x & 15) : 0, hi = wd == whi ? ((r.x + r.y - 1) & 15) + 1 : 16;
      atomicOr(&s_mask[w][slot], ((1u << hi) - 1u) & ~((1u << lo) - 1u));
    }
  }
  __syncthreads();
  int2 d = make_int2(s_word[w][lane], (int)s_mask[w][lane]);
  if (!fits) d = make_int2(0, (real && lane == 0) ? -1 : 0);
  if (b < nblocks_padded) chunks[b * kClassChunks + lane] = d;
}

// AND of the sign codes of the vertices a run table lists (RUNS slots of (start, length), one per lane; length 0: unused,
// -1 in slot 0: no summary -> 0).  The elements are numbered through (prefix sums of the lengths) and dealt to the lanes E
// at a time, so that a lane's loads are independent and in flight together: walking the runs one after the other left
// every wavefront ~12 dependent load latencies long.
template <int RUNS, int E>
__device__ __forceinline__ unsigned class_runs_and(const int2* __restrict__ table, const uint8_t* __restrict__ code, int lane)
{
  const int2 mine = lane < RUNS ? table[lane] : make_int2(0, 0);
  const bool summary = __shfl(mine.y, 0, 64) >= 0;
  const int nr = summary ? __popcll(__ballot(mine.y > 0)) : 0;
  unsigned all = summary ? 3u : 0u;
  const int incl = wave_inclusive_scan<int>(summary ? mine.y : 0);
  const int total = __shfl(incl, 63, 64);
  for (int t0 = 0; t0 < total; t0 += 64 * E)
  {
    int addr[E];
#pragma unroll
    for (int e = 0; e < E; ++e) addr[e] = -1;
    for (int j = 0; j < nr; ++j)
    {
      const int start = __shfl(mine.x, j, 64), hi = __shfl(incl, j, 64), lo = hi - __shfl(mine.y, j, 64);
#pragma unroll
      for (int e = 0; e < E; ++e)
      {
        const int t = t0 + lane + 64 * e;
        addr[e] = (t >= lo && t < hi) ? start + (t - lo) : addr[e];
      }
    }
    unsigned v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = addr[e] >= 0 ? (unsigned)code[addr[e]] : 3u;
#pragma unroll
    for (int e = 0; e < E; ++e) all &= v[e];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) all &= __shfl_xor(all, o, 64);
  return all;
}

// CELLS equal domain bytes from cbase on, written by the wavefront
template <int CELLS>
__device__ __forceinline__ void class_fill(int8_t* __restrict__ domain, int64_t cbase, int64_t ncells, int8_t d, int lane)
{
  const uint32_t w4 = 0x01010101u * (uint32_t)(uint8_t)d;
  // 16 B per lane when the run is whole and aligned: one store instruction per 1024 cells.  (The kernel is not bound by
  // its stores -- 0.78 -> 0.75 ms with every block uniform -- nor helped by a persistent grid with the next block's
  // runs prefetched: 1.5 ms.  Round 5 read that as "786 k short wavefronts live on how many of them are in flight";
  // round 12 found the other half: the wavefronts were not short.  Decoding the runs cost ~1200 issued instructions per
  // pair of blocks, and with the decode gone -- class_chunks_and2 -- the all-uniform case went from 0.51 to 0.26 ms at
  // 512^3, the time its bytes take at the rate fill16_kernel streams at.)
  if (cbase + CELLS <= ncells && (reinterpret_cast<uintptr_t>(domain + cbase) & 15) == 0)
  {
    if (lane < CELLS / 16) reinterpret_cast<uint4*>(domain + cbase)[lane] = make_uint4(w4, w4, w4, w4);
    return;
  }
#pragma unroll
  for (int q4 = 0; q4 < CELLS / 256; ++q4)
  {
    const int64_t c = cbase + 4 * (lane + 64 * q4);
    if (c + 4 <= ncells && (reinterpret_cast<uintptr_t>(domain + c) & 3) == 0) *reinterpret_cast<uint32_t*>(domain + c) = w4;
    else
      for (int64_t q = c; q < c + 4 && q < ncells; ++q) domain[q] = d;
  }
}

// The same for TWO tables at once (lanes 0..31 hold the runs of table A, lanes 32..63 those of table B; RUNS <= 32): both
// tables arrive with one load latency and both sets of sign codes with a second one: a wavefront that decides two
// blocks halves the number of wavefronts (786 k at 512^3, two dependent loads each).  What this decoder costs beside
// its loads -- a scan, and per run and address a compare-and-select chain in a loop the compiler treats as divergent --
// is repeated every step for runs that never change: it is the path of CFX_CLASSIFY_CHUNKS=0 and of code arrays that
// are not 16 B aligned now; class_chunks_and2 reads the same bytes through a table built once per mesh.
template <int RUNS, int E>
__device__ __forceinline__ void class_runs_and2(const int2* __restrict__ tableA, const int2* __restrict__ tableB, bool haveB,
                                                const uint8_t* __restrict__ code, int lane, unsigned& allA, unsigned& allB)
{
  static_assert(RUNS <= 32, "two tables in one wavefront");
  const int half = lane >> 5, hl = lane & 31;
  int2 mine = make_int2(0, 0);
  if (hl < RUNS && (half == 0 || haveB)) mine = (half == 0 ? tableA : tableB)[hl];
  const bool sumA = __shfl(mine.y, 0, 64) >= 0, sumB = haveB && __shfl(mine.y, 32, 64) >= 0;
  const unsigned long long pos = __ballot(mine.y > 0);
  const int nrA = sumA ? __popcll(pos & 0xffffffffull) : 0, nrB = sumB ? __popcll(pos >> 32) : 0;
  const bool mysum = half == 0 ? sumA : sumB;
  int incl = wave_inclusive_scan<int>(mysum ? mine.y : 0);
  const int totA = __shfl(incl, 31, 64);
  const int totB = __shfl(incl, 63, 64) - totA;
  if (half) incl -= totA; // prefix inside the own table
  allA = sumA ? 3u : 0u; allB = sumB ? 3u : 0u;
  const int total = max(totA, totB);
  for (int t0 = 0; t0 < total; t0 += 64 * E)
  {
    int addrA[E], addrB[E];
#pragma unroll
    for (int e = 0; e < E; ++e) { addrA[e] = -1; addrB[e] = -1; }
    for (int j = 0; j < max(nrA, nrB); ++j)
    {
      const int sa = __shfl(mine.x, j, 64), ha = __shfl(incl, j, 64), la = ha - __shfl(mine.y, j, 64);
      const int sb = __shfl(mine.x, 32 + j, 64), hb = __shfl(incl, 32 + j, 64), lb = hb - __shfl(mine.y, 32 + j, 64);
#pragma unroll
      for (int e = 0; e < E; ++e)
      {
        const int t = t0 + lane + 64 * e;
        addrA[e] = (j < nrA && t >= la && t < ha) ? sa + (t - la) : addrA[e];
        addrB[e] = (j < nrB && t >= lb && t < hb) ? sb + (t - lb) : addrB[e];
      }
    }
    unsigned va[E], vb[E];
#pragma unroll
    for (int e = 0; e < E; ++e) va[e] = addrA[e] >= 0 ? (unsigned)code[addrA[e]] : 3u;
#pragma unroll
    for (int e = 0; e < E; ++e) vb[e] = addrB[e] >= 0 ? (unsigned)code[addrB[e]] : 3u;
#pragma unroll
    for (int e = 0; e < E; ++e) { allA &= va[e]; allB &= vb[e]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { allA &= __shfl_xor(allA, o, 64); allB &= __shfl_xor(allB, o, 64); }
}

// AND of the bytes of a 16 B word of sign codes whose bit is set in mask (bit i: byte i); the other bytes count as 0xff.
// (nibble -> byte mask: the four shifted copies of the nibble do not overlap, so bit k lands alone at bit 8 k)
__device__ __forceinline__ unsigned class_word_and(const uint4 w, unsigned mask)
{
  auto keep = [](unsigned v, unsigned nib) { return v | ~((((nib & 15u) * 0x00204081u) & 0x01010101u) * 0xffu); };
  unsigned a = keep(w.x, mask) & keep(w.y, mask >> 4) & keep(w.z, mask >> 8) & keep(w.w, mask >> 12);
  a &= a >> 16;
  return a & (a >> 8);
}

// The block decision of a pair of blocks from their chunk descriptors (cfx_mesh_s::class_chunks: mesh-static, where the
// run tables had to be scanned and decoded into byte addresses by every wavefront of every step): one 16 B load of two
// descriptors per lane -- lanes 0..31 those of block A, 32..63 those of block B, 1 KB of one stream --, two 16 B loads of
// sign codes per lane (an unused descriptor names word 0 with an empty mask: no branch around the load), the masked
// AND, and two ballots for the reduction over each half.  Exactly the bytes of the runs take part, as in
// class_runs_and2.  A flagged block (no summary, or more than kClassChunks words) takes the run decoder.
// code starts on a 16 B boundary and its allocation covers whole words (checked at the launch).
template <int RUNS, int E>
__device__ __forceinline__ void class_chunks_and2(const int2* __restrict__ chunks, const int2* __restrict__ tableA, bool haveB,
                                                  const uint8_t* __restrict__ code, int lane, unsigned& allA, unsigned& allB)
{
  const int4 d = reinterpret_cast<const int4*>(chunks)[lane];
  const bool flagA = __builtin_amdgcn_readlane(d.y, 0) < 0, flagB = haveB && __builtin_amdgcn_readlane(d.y, 32) < 0;
  const uint4* __restrict__ words = reinterpret_cast<const uint4*>(code);
  const uint4 w0 = words[d.x], w1 = words[d.z];
  const unsigned acc = class_word_and(w0, (unsigned)d.y) & class_word_and(w1, (unsigned)d.w);
  const unsigned long long no1 = __ballot((acc & 1u) == 0u), no2 = __ballot((acc & 2u) == 0u);
  allA = ((no1 & 0xffffffffull) == 0 ? 1u : 0u) | ((no2 & 0xffffffffull) == 0 ? 2u : 0u);
  allB = ((no1 >> 32) == 0 ? 1u : 0u) | ((no2 >> 32) == 0 ? 2u : 0u);
  if (flagA) allA = class_runs_and<RUNS, E>(tableA, code, lane);
  if (flagB) allB = class_runs_and<RUNS, E>(tableA + RUNS, code, lane);
}

// AND of the sign codes over the 16 B words that the spans of a quarter table lie in (kClassSubRuns spans, four lanes per
// span, a word per lane and round: spans of up to 64 ids in one round).  The spans are supersets of the quarter's
// vertices already, so the bytes of their first and last word that lie outside them take part as well: a quarter they
// turn mixed goes cell by cell, which gives the same cells the same classes.  Pad bytes behind the last dof likewise.
// code starts on a 16 B boundary and its allocation covers whole words (checked at the launch).
__device__ __forceinline__ unsigned class_spans_and_words(const int2* __restrict__ table, const uint8_t* __restrict__ code, int lane)
{
  static_assert(kClassSubRuns * 4 == 64, "four lanes per span");
  const int2 s = table[lane >> 2];
  if (__builtin_amdgcn_readlane(s.y, 0) < 0) return 0u; // no summary
  const uint4* __restrict__ words = reinterpret_cast<const uint4*>(code);
  const int last = s.y > 0 ? (s.x + s.y - 1) >> 4 : -1;
  unsigned acc = 0xffffffffu;
  for (int w = (s.x >> 4) + (lane & 3); __any(w <= last); w += 4)
    if (w <= last)
    {
      const uint4 v = words[w];
      acc &= v.x & v.y & v.z & v.w;
    }
  acc &= acc >> 16;
  acc &= acc >> 8;
  const unsigned long long no1 = __ballot((acc & 1u) == 0u), no2 = __ballot((acc & 2u) == 0u);
  return (no1 == 0 ? 1u : 0u) | (no2 == 0 ? 2u : 0u);
}

// one quarter of a block with vertices on both sides (or on the interface): decided whole from its table where its
// vertices have one sign, cell by cell (classify_kernel) otherwise.  The whole wavefront works on the one quarter; n_in
// and n_cut take its inside / cut cells, spread over the lanes.  (WORDS: the decision from whole 16 B words, as the
// block's own from its chunk descriptors; otherwise from the run decoder.)
template <int ND, bool WORDS>
__device__ __forceinline__ void classify_quarter(int64_t ncells, int64_t b, int sq, const int32_t* __restrict__ dofmap,
                                                 const int2* __restrict__ sub_runs, const uint8_t* __restrict__ code,
                                                 int8_t* __restrict__ domain, uint8_t* __restrict__ touch, int lane, int& n_in, int& n_cut)
{
  constexpr int SUB = kClassBlock / kClassSub, U = SUB / 64;
  const int64_t sbase = b * kClassBlock + (int64_t)sq * SUB;
  const int2* table = sub_runs + (b * kClassSub + sq) * kClassSubRuns;
  unsigned sall;
  if constexpr (WORDS) sall = class_spans_and_words(table, code, lane);
  else sall = class_runs_and<kClassSubRuns, 4>(table, code, lane);
  if (sall == 1u || sall == 2u)
  {
    class_fill<SUB>(domain, sbase, ncells, sall == 1u ? (int8_t)CFX_INSIDE : (int8_t)CFX_OUTSIDE, lane);
    if (sall == 1u && lane == 0) n_in += (int)(ncells - sbase < SUB ? ncells - sbase : SUB);
    return;
  }
  int32_t d[U][ND];
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    const int64_t c = sbase + lane + (int64_t)u * 64;
    if (c >= ncells) continue;
    if constexpr (ND == 4)
    {
      const int4 v = *reinterpret_cast<const int4*>(dofmap + c * 4);
      d[u][0] = v.x; d[u][1] = v.y; d[u][2] = v.z; d[u][3] = v.w;
    }
    else
    {
#pragma unroll
      for (int i = 0; i < ND; ++i) d[u][i] = dofmap[c * ND + i];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
  {
    const int64_t c = sbase + lane + (int64_t)u * 64;
    if (c >= ncells) continue;
    unsigned a = 3u;
#pragma unroll
    for (int i = 0; i < ND; ++i) a &= code[d[u][i]];
    domain[c] = a == 1u ? (int8_t)CFX_INSIDE : (a == 2u ? (int8_t)CFX_OUTSIDE : (int8_t)CFX_INTERSECTED);
    n_in += a == 1u ? 1 : 0;
    n_cut += (a != 1u && a != 2u) ? 1 : 0;
    if (touch && a != 1u && a != 2u) // (a cut cell: its dofs are next to the interface; every writer stores 1)
    {
#pragma unroll
      for (int i = 0; i < ND; ++i) touch[d[u][i]] = 1;
    }
  }
}

// a block with vertices on both sides (or on the interface): quarter by quarter.  The whole wavefront works on the one
// block.
template <int ND, bool WORDS>
__device__ __forceinline__ void classify_block_mixed(int64_t ncells, int64_t b, const int32_t* __restrict__ dofmap,
                                                     const int2* __restrict__ sub_runs, const uint8_t* __restrict__ code,
                                                     int8_t* __restrict__ domain, int32_t* tiles_inside, int32_t* tiles_cut,
                                                     uint8_t* __restrict__ touch, int lane)
{
  constexpr int SUB = kClassBlock / kClassSub;
  const int64_t cbase = b * kClassBlock;
  const int64_t tile = cbase / kByteTile;
  int n_in = 0, n_cut = 0;
  // (the four quarter tables decided in one go -- 16 lanes per table, one round of loads -- measured in round 5: no change,
  // 1.056 against 1.044 ms at 512^3: the mixed blocks live on their cell loops)
  for (int sq = 0; sq < kClassSub; ++sq)
  {
    if (cbase + (int64_t)sq * SUB >= ncells) break;
    classify_quarter<ND, WORDS>(ncells, b, sq, dofmap, sub_runs, code, domain, touch, lane, n_in, n_cut);
  }
  if (tiles_inside)
  {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n_in += __shfl_xor(n_in, o, 64); n_cut += __shfl_xor(n_cut, o, 64); }
    if (lane == 0)
    {
      if (n_in) atomicAdd(&tiles_inside[tile], n_in);
      if (n_cut) atomicAdd(&tiles_cut[tile], n_cut);
    }
  }
}

// one wavefront per PAIR of blocks of kClassBlock cells
#ifndef CFX_CLASSIFY_WAVES
#define CFX_CLASSIFY_WAVES 5 // (round 5, two blocks per wavefront, 512^3 sphere: 4 -> 1.21 ms, 5 -> 1.04, 6 -> 1.09)
#endif
#ifndef CFX_CLASSIFY_E
#define CFX_CLASSIFY_E 12 // sign codes per lane, table and round of loads (a block has ~690: one round)
#endif
// (CHUNKS: the block decision from the chunk descriptors; otherwise, and for the blocks the descriptors flag, from the runs)
template <int ND, bool CHUNKS>
__global__ void __launch_bounds__(kBlock, CFX_CLASSIFY_WAVES) classify_culled_kernel(int64_t ncells, int64_t nblocks, const int32_t* __restrict__ dofmap,
                                                                 const int2* __restrict__ runs, const int2* __restrict__ chunks,
                                                                 const int2* __restrict__ sub_runs,
                                                                 const uint8_t* __restrict__ code, int8_t* __restrict__ domain,
                                                                 int32_t* tiles_inside, int32_t* tiles_cut,
                                                                 uint8_t* __restrict__ block_class, uint8_t* __restrict__ touch)
{
  static_assert(kByteTile % kClassBlock == 0, "classification blocks must nest in compaction tiles");
  const int lane = threadIdx.x & 63;
  const int64_t b0 = 2 * ((int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
  if (b0 >= nblocks) return;
  const bool have1 = b0 + 1 < nblocks;
  unsigned all[2];
  if constexpr (CHUNKS)
    class_chunks_and2<kClassRuns, CFX_CLASSIFY_E>(chunks + b0 * kClassChunks, runs + b0 * kClassRuns, have1, code, lane, all[0], all[1]);
  else
    class_runs_and2<kClassRuns, CFX_CLASSIFY_E>(runs + b0 * kClassRuns, runs + (b0 + 1) * kClassRuns, have1, code, lane, all[0], all[1]);
  for (int k = 0; k < (have1 ? 2 : 1); ++k)
  {
    const int64_t b = b0 + k;
    const int64_t cbase = b * kClassBlock;
    const unsigned a = all[k];
    if (a == 1u || a == 2u)
    {
      // every vertex of the block on one side
      class_fill<kClassBlock>(domain, cbase, ncells, a == 1u ? (int8_t)CFX_INSIDE : (int8_t)CFX_OUTSIDE, lane);
      if (tiles_inside && a == 1u && lane == 0)
        atomicAdd(&tiles_inside[cbase / kByteTile], (int32_t)(ncells - cbase < kClassBlock ? ncells - cbase : kClassBlock));
      if (block_class && lane == 0) block_class[b] = (uint8_t)a;
      continue;
    }
    if (block_class && lane == 0) block_class[b] = 0;
    classify_block_mixed<ND, CHUNKS>(ncells, b, dofmap, sub_runs, code, domain, tiles_inside, tiles_cut, touch, lane);
  }
}

// Implicit-structured variant of a1 for the generated box / slab meshes with the level set on the geometry dofmap
// (CFX_IMPLICIT_BOX=1): the connectivity of a Kuhn-split cube is a function of the cube index, so one thread
// classifies the cells of a cube from its 2^tdim corner codes and the 12.9 GB connectivity stream of
// classify_kernel (16 of its 18.3 algorithmic bytes per cell) is not read at all.  Same domain array.
template <int TDIM>
__global__ void __launch_bounds__(kBlock) classify_box_kernel(int64_t ncubes, int n, const uint8_t* __restrict__ code,
                                                              int8_t* __restrict__ domain, int32_t* tiles_inside,
                                                              int32_t* tiles_cut, uint8_t* __restrict__ touch)
{
  constexpr int NC = TDIM == 3 ? 6 : 2; // cells per cube
  constexpr int NV = TDIM + 1;
  // corners of the Kuhn simplices, local corner i = bx + 2 by + 4 bz (the generator's tables, cfx_mesh.hip)
  constexpr int tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
  constexpr int tri[2][3] = {{0, 1, 3}, {0, 3, 2}};
  __shared__ int8_t s_dom[kBlock * NC];
  __shared__ int s_cnt[4]; // inside / cut cells of the block in the two compaction tiles it can overlap
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t tile0 = ((int64_t)blockIdx.x * kBlock * NC) / kByteTile;
  if (h < ncubes)
  {
    const int64_t n1 = n + 1;
    const int64_t ix = h % n, iy = (h / n) % n, iz = TDIM == 3 ? h / ((int64_t)n * n) : 0;
    const int64_t v0 = ix + n1 * (iy + n1 * iz);
    unsigned c[1 << TDIM];
#pragma unroll
    for (int i = 0; i < (1 << TDIM); ++i)
      c[i] = code[v0 + (i & 1) + n1 * (((i >> 1) & 1) + n1 * ((i >> 2) & 1))];
#pragma unroll
    for (int k = 0; k < NC; ++k)
    {
      unsigned all = 3u;
#pragma unroll
      for (int j = 0; j < NV; ++j) all &= c[TDIM == 3 ? tet[k][j] : tri[k][j]];
      s_dom[threadIdx.x * NC + k] = all == 1u ? (int8_t)CFX_INSIDE : (all == 2u ? (int8_t)CFX_OUTSIDE : (int8_t)CFX_INTERSECTED);
      if (touch && all != 1u && all != 2u) // (a cut cell: its vertices are next to the interface; every writer stores 1)
      {
#pragma unroll
        for (int j = 0; j < NV; ++j)
        {
          const int i = TDIM == 3 ? tet[k][j] : tri[k][j];
          touch[v0 + (i & 1) + n1 * (((i >> 1) & 1) + n1 * ((i >> 2) & 1))] = 1;
        }
      }
      if (tiles_inside && all != 2u)
        atomicAdd(&s_cnt[2 * (int)((h * NC + k) / kByteTile - tile0) + (all == 1u ? 0 : 1)], 1);
    }
  }
  __syncthreads();
  if (tiles_inside && threadIdx.x < 4 && s_cnt[threadIdx.x])
    atomicAdd((threadIdx.x & 1 ? tiles_cut : tiles_inside) + tile0 + (threadIdx.x >> 1), s_cnt[threadIdx.x]);
  // the block's cells are contiguous: coalesced byte stores out of LDS
  const int64_t first = (int64_t)blockIdx.x * kBlock * NC;
  const int64_t count = min((int64_t)kBlock, ncubes - (int64_t)blockIdx.x * kBlock) * NC;
  for (int i = threadIdx.x; i < count; i += kBlock) domain[first + i] = s_dom[i];
}

// ---------------------------------------------------------------------------
// a7 ghost-penalty band.  For every cut cell c (ascending) and local facet lf:
// the neighbour n across the facet is found through the vertex->cells
// incidence; the facet is kept when n exists, n is in (cut U selected) and --
// if n is itself cut -- c < n, so each facet is emitted once, by its smallest
// cut cell.  Row = (c0, lf0, c1, lf1) with c0 < c1.
// (python/cutfemx/cut.py:340-380, python/cutfemx/wrappers/cut.cpp:84-114)
// ---------------------------------------------------------------------------
template <int TDIM>
__device__ __forceinline__ bool facet_neighbour(const int32_t* __restrict__ conn, const int64_t* __restrict__ v2c_off,
                                                const int32_t* __restrict__ v2c, int64_t c, int lf, int32_t& nb,
                                                int& nb_lf)
{
  constexpr int NV = TDIM + 1;
  int32_t cv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) cv[i] = conn[c * NV + i];
  // pivot = first facet vertex
  int32_t pivot = -1;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i != lf && pivot < 0) pivot = cv[i];
  for (int64_t k = v2c_off[pivot]; k < v2c_off[pivot + 1]; ++k)
  {
    const int32_t o = v2c[k];
    if (o == c) continue;
    int32_t ov[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) ov[i] = conn[(int64_t)o * NV + i];
    // o shares the facet iff all facet vertices of c are vertices of o
    bool all = true;
#pragma unroll
    for (int i = 0; i < NV; ++i)
    {
      if (i == lf) continue;
      bool found = false;
#pragma unroll
      for (int j = 0; j < NV; ++j) found = found || (ov[j] == cv[i]);
      all = all && found;
    }
    if (!all) continue;
    // local facet of o = its vertex that is not on the facet
    int olf = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j)
    {
      bool onf = false;
#pragma unroll
      for (int i = 0; i < NV; ++i) onf = onf || (i != lf && cv[i] == ov[j]);
      if (!onf) olf = j;
    }
    nb = o; nb_lf = olf;
    return true;
  }
  return false;
}

// One thread per (cut cell, local facet): the neighbour search (a scan of the vertex->cells list of a
// facet vertex) runs once, its result is parked in `cand` and packed in cell / facet order afterwards.
// neighbour of cell c across local facet lf from the mesh's cell->cell table; nb_lf = the vertex of the
// neighbour that is not on the facet
template <int TDIM>
__device__ __forceinline__ bool facet_neighbour_tab(const int32_t* __restrict__ conn, const int32_t* __restrict__ c2c,
                                                    int64_t c, int lf, int32_t& nb, int& nb_lf)
{
  constexpr int NV = TDIM + 1;
  nb = c2c[c * NV + lf];
  if (nb < 0) return false;
  int32_t cv[NV], ov[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { cv[i] = conn[c * NV + i]; ov[i] = conn[(int64_t)nb * NV + i]; }
  nb_lf = 0;
#pragma unroll
  for (int j = 0; j < NV; ++j)
  {
    bool onf = false;
#pragma unroll
    for (int i = 0; i < NV; ++i) onf = onf || (i != lf && cv[i] == ov[j]);
    if (!onf) nb_lf = j;
  }
  return true;
}

template <int TDIM, bool XCD>
__global__ void __launch_bounds__(kBlock) cell_neighbours_kernel(int64_t ncells, const int32_t* __restrict__ conn,
                                                                 const int64_t* __restrict__ v2c_off,
                                                                 const int32_t* __restrict__ v2c, int32_t* __restrict__ c2c)
{
  constexpr int NV = TDIM + 1;
  // (XCD: every XCD -- every L2 -- walks one contiguous chunk of the cells; the candidates of neighbouring cells are
  // the same rows of the connectivity: 95 -> 86 ms at 512^3)
  const int64_t c = (XCD ? xcd_block_id() : (int64_t)blockIdx.x) * kBlock + threadIdx.x;
  if (c >= ncells) return;
  // All facets of the cell from TWO incidence lists instead of one list per facet: a cell that shares NV - 1
  // vertices with c is its neighbour across the facet opposite the vertex it lacks; every facet but the one opposite
  // vertex 0 contains vertex 0 (candidates: the cells around vertex 0), that one contains vertex 1.
  // (Measured and dropped in round 4: deciding from the incidence lists alone -- a candidate is the neighbour across
  // facet i when it is in the lists of all vertices but vertex i, one binary search per (candidate, vertex) instead of
  // the candidate's connectivity row -- ran 5.6 x slower: 530 ms, ~600 dependent 4 B loads per cell.)
  int32_t cv[NV], out[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { cv[i] = conn[c * NV + i]; out[i] = -1; }
  constexpr int KB = 4; // candidates in flight: ids first, then their connectivity rows, then the compares
#pragma unroll
  for (int pass = 0; pass < 2; ++pass)
  {
    const int32_t pivot = cv[pass];
    const int64_t kb = v2c_off[pivot], ke = v2c_off[pivot + 1];
    for (int64_t k0 = kb; k0 < ke; k0 += KB)
    {
      int32_t o[KB], ov[KB][NV];
#pragma unroll
      for (int u = 0; u < KB; ++u) o[u] = v2c[k0 + u < ke ? k0 + u : ke - 1];
#pragma unroll
      for (int u = 0; u < KB; ++u)
      {
        if constexpr (NV == 4)
        {
          const int4 q = *reinterpret_cast<const int4*>(conn + (int64_t)o[u] * 4);
          ov[u][0] = q.x; ov[u][1] = q.y; ov[u][2] = q.z; ov[u][3] = q.w;
        }
        else
        {
#pragma unroll
          for (int i = 0; i < NV; ++i) ov[u][i] = conn[(int64_t)o[u] * NV + i];
        }
      }
#pragma unroll
      for (int u = 0; u < KB; ++u)
      {
        if (k0 + u >= ke || o[u] == c) continue;
        int shared = 0, missing = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i)
        {
          bool found = false;
#pragma unroll
          for (int j = 0; j < NV; ++j) found = found || (ov[u][j] == cv[i]);
          shared += found ? 1 : 0;
          missing = found ? missing : i;
        }
        // pass 0 settles the facets that contain vertex 0, pass 1 the one opposite to it
        if (shared == NV - 1 && (pass == 0 ? missing != 0 : missing == 0))
        {
#pragma unroll
          for (int i = 0; i < NV; ++i) out[i] = (i == missing && out[i] < 0) ? o[u] : out[i];
        }
      }
    }
  }
  if constexpr (NV == 4) *reinterpret_cast<int4*>(c2c + c * 4) = make_int4(out[0], out[1], out[2], out[3]);
  else
  {
#pragma unroll
    for (int i = 0; i < NV; ++i) c2c[c * NV + i] = out[i];
  }
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) ghost_facets_find_kernel(DevN ncut_d, const int32_t* __restrict__ cut_cells,
                                                                   const int32_t* __restrict__ conn,
                                                                   const int32_t* __restrict__ c2c,
                                                                   const int8_t* __restrict__ domain, SelectorPred sel,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ cand)
{
  const int64_t ncut = dev_n(ncut_d);
  constexpr int NV = TDIM + 1;
  // one thread per cut cell: its NV facets one after the other, the count written once (no counter to zero first: a
  // launch less per step -- a kernel boundary costs ~10 us here)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncut)
  {
    if (i < ncut_d.cap) counts[i] = 0; // (list shorter than its capacity: the scan runs over the capacity)
    return;
  }
  const int64_t c = cut_cells[i];
  int n = 0;
#pragma unroll
  for (int lf = 0; lf < NV; ++lf)
  {
    int4 r = make_int4(-1, -1, -1, -1);
    int32_t nb;
    int nlf;
    if (facet_neighbour_tab<TDIM>(conn, c2c, c, lf, nb, nlf))
    {
      const bool nb_cut = domain[nb] == CFX_INTERSECTED;
      if ((nb_cut || sel(nb)) && !(nb_cut && nb < c))
      {
        r = (c < nb) ? make_int4((int)c, lf, nb, nlf) : make_int4(nb, nlf, (int)c, lf);
        ++n;
      }
    }
    *reinterpret_cast<int4*>(cand + 4 * (i * NV + lf)) = r;
  }
  counts[i] = n;
}

template <int TDIM>
__global__ void __launch_bounds__(kBlock) ghost_facets_pack_kernel(DevN ncut_d, const int32_t* __restrict__ cand,
                                                                   const int64_t* __restrict__ offs,
                                                                   int32_t* __restrict__ rows)
{
  const int64_t ncut = dev_n(ncut_d);
  constexpr int NV = TDIM + 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= ncut) return;
  int64_t o = offs[i];
#pragma unroll
  for (int lf = 0; lf < NV; ++lf)
  {
    const int4 r = *reinterpret_cast<const int4*>(cand + 4 * (i * NV + lf));
    if (r.x >= 0) { *reinterpret_cast<int4*>(rows + 4 * o) = r; ++o; }
  }
}

// ---------------------------------------------------------------------------
// 8f-3 cell aggregation (cell_aggregation.cpp:143-270) without its sequential sweeps.
// Sweep k of the reference visits the unrooted cut cells in ascending order; cell c takes the
// first (ascending) active neighbour that is rooted AT THAT MOMENT: a root, a cell rooted in an
// earlier sweep, or a lower-numbered cell rooted earlier in this sweep.  Hence the sweep t(c) in
// which c is rooted is the least fixed point of
//     t(c) = max(0, min over active neighbours o of t(o) + [o > c]),   t(root) = -1,
// a shortest-path problem with 0/1 edge weights solved by parallel relaxation; the neighbour
// chosen in sweep t(c) is the first o with t(o) < t(c) or (t(o) == t(c) and o < c); roots,
// aggregate ids and depths then follow the parent pointers (pointer jumping).
// ---------------------------------------------------------------------------
constexpr int32_t kAggUnset = 0x7fffffff;

template <int TDIM>
__device__ __forceinline__ int sorted_neighbours(const int32_t* __restrict__ conn, const int64_t* __restrict__ v2c_off,
                                                 const int32_t* __restrict__ v2c, int64_t c, int32_t* nbs)
{
  int n = 0;
  for (int lf = 0; lf <= TDIM; ++lf)
  {
    int32_t nb;
    int nlf;
    if (facet_neighbour<TDIM>(conn, v2c_off, v2c, c, lf, nb, nlf)) nbs[n++] = nb;
  }
  for (int a = 1; a < n; ++a) // insertion sort, n <= 4
  {
    const int32_t v = nbs[a];
    int b = a - 1;
    while (b >= 0 && nbs[b] > v) { nbs[b + 1] = nbs[b]; --b; }
    nbs[b + 1] = v;
  }
  return n;
}

// selected volume fraction of the cut cells from order-1 volume rules
template <int TDIM>
__global__ void agg_fraction_kernel(int64_t nr, const int32_t* __restrict__ offsets, const int32_t* __restrict__ parent,
                                    const double* __restrict__ weights, const double* __restrict__ x,
                                    const int32_t* __restrict__ conn, double* fraction)
{
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nr) return;
  double s = 0.0;
  for (int32_t q = offsets[e]; q < offsets[e + 1]; ++q) s += weights[q];
  Geo<TDIM> g;
  load_cell<TDIM>(x, conn, parent[e], g);
  jacobian<TDIM>(g);
  atomicAdd(&fraction[parent[e]], s / (fabs(g.detJ) / (TDIM == 2 ? 2.0 : 6.0)));
}

// cls bits: 1 interior, 2 cut, 4 well posed (root), 8 ill posed
__global__ void agg_init_kernel(int64_t nc, const int8_t* __restrict__ domain, int8_t selcode, int policy,
                                const double* __restrict__ fraction, double threshold, int32_t* t, uint8_t* cls)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const bool interior = domain[c] == selcode, cutc = domain[c] == CFX_INTERSECTED;
  const bool well = interior || (cutc && policy == 1 && fraction[c] >= threshold);
  t[c] = well ? -1 : kAggUnset;
  cls[c] = (uint8_t)((interior ? 1 : 0) | (cutc ? 2 : 0) | (well ? 4 : 0) | ((cutc && !well) ? 8 : 0));
}

template <int TDIM>
__global__ void agg_relax_kernel(int64_t n_ill, const int32_t* __restrict__ ill, const int32_t* __restrict__ conn,
                                 const int64_t* __restrict__ v2c_off, const int32_t* __restrict__ v2c,
                                 const uint8_t* __restrict__ cls, int32_t* t, int* changed)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ill) return;
  const int32_t c = ill[i];
  int32_t nbs[TDIM + 1];
  const int n = sorted_neighbours<TDIM>(conn, v2c_off, v2c, c, nbs);
  int32_t best = kAggUnset;
  for (int k = 0; k < n; ++k)
  {
    const int32_t o = nbs[k];
    if (!(cls[o] & 3)) continue; // active cells only
    const int32_t to = *reinterpret_cast<volatile int32_t*>(&t[o]);
    if (to == kAggUnset) continue;
    const int32_t cand = to + (o > c ? 1 : 0);
    best = cand < best ? cand : best;
  }
  if (best != kAggUnset && best < 0) best = 0;
  if (best < t[c]) { t[c] = best; *changed = 1; }
}

template <int TDIM>
__global__ void agg_parent_kernel(int64_t n_ill, const int32_t* __restrict__ ill, const int32_t* __restrict__ conn,
                                  const int64_t* __restrict__ v2c_off, const int32_t* __restrict__ v2c,
                                  const uint8_t* __restrict__ cls, const int32_t* __restrict__ t, int64_t limit,
                                  int32_t* parent)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ill) return;
  const int32_t c = ill[i];
  int32_t p = -1;
  const int32_t tc = t[c];
  if (tc != kAggUnset && (int64_t)tc < limit)
  {
    int32_t nbs[TDIM + 1];
    const int n = sorted_neighbours<TDIM>(conn, v2c_off, v2c, c, nbs);
    for (int k = 0; k < n && p < 0; ++k)
    {
      const int32_t o = nbs[k];
      if (!(cls[o] & 3) || t[o] == kAggUnset) continue;
      if (t[o] < tc || (t[o] == tc && o < c)) p = o;
    }
  }
  parent[i] = p;
}

__global__ void agg_roots_kernel(int64_t n_well, const int32_t* __restrict__ well, int32_t* root, int32_t* agg,
                                 int32_t* depth)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_well) return;
  const int32_t c = well[i];
  root[c] = c; agg[c] = (int32_t)i; depth[c] = 0; // aggregate ids follow the ascending root order (:211-217)
}

__global__ void agg_resolve_kernel(int64_t n_ill, const int32_t* __restrict__ ill, const int32_t* __restrict__ parent,
                                   int32_t* root, int32_t* agg, int32_t* depth, int* changed)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ill) return;
  const int32_t c = ill[i], p = parent[i];
  if (p < 0 || root[c] >= 0) return;
  const int32_t rp = *reinterpret_cast<volatile int32_t*>(&root[p]);
  if (rp < 0) return;
  // the parent's three fields were written before its root became visible only within one
  // thread; read depth/aggregate after the root and re-run until nothing changes
  depth[c] = depth[p] + 1; agg[c] = agg[p];
  __threadfence();
  root[c] = rp;
  *changed = 1;
}

__global__ void agg_flag_rootless_kernel(int64_t n_ill, const int32_t* __restrict__ ill, const int32_t* __restrict__ root,
                                         uint8_t* cls)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ill && root[ill[i]] < 0) cls[ill[i]] |= 16;
}

__global__ void agg_pairs_kernel(int64_t n, const int32_t* __restrict__ bad, const int32_t* __restrict__ root,
                                 int32_t* rows)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) *reinterpret_cast<int4*>(rows + 4 * i) = make_int4(bad[i], 0, root[bad[i]], 0);
}

struct ClsMask
{
  const uint8_t* cls;
  uint8_t any, none;
  __device__ bool operator()(int64_t c) const { return (cls[c] & any) != 0 && (cls[c] & none) == 0; }
};

// cells outside a candidate subset: a classification code no selector matches
__global__ void restrict_domain_kernel(int64_t n, const uint8_t* __restrict__ keep, int8_t* __restrict__ domain)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n && !keep[c]) domain[c] = (int8_t)CFX_NOT_CANDIDATE;
}

__global__ void mark_subset_kernel(int64_t n, const int32_t* __restrict__ cells, int64_t ncells, uint8_t* keep, int* bad)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cells[i];
  if (c < 0 || c >= ncells) { *bad = 1; return; }
  keep[c] = 1;
}

// interior facets inside a cell set: thread per (listed cell, facet), emitted from the lower cell
template <int TDIM>
__global__ void __launch_bounds__(kBlock) interior_facets_find_kernel(int64_t n, const int32_t* __restrict__ cells,
                                                                      const int32_t* __restrict__ conn,
                                                                      const int64_t* __restrict__ v2c_off,
                                                                      const int32_t* __restrict__ v2c,
                                                                      const uint8_t* __restrict__ inset,
                                                                      int32_t* __restrict__ counts, int32_t* __restrict__ cand)
{
  constexpr int NV = TDIM + 1;
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n * NV) return;
  const int64_t i = t / NV;
  const int lf = (int)(t - i * NV);
  const int64_t c = cells[i];
  int4 r = make_int4(-1, -1, -1, -1);
  int32_t nb;
  int nlf;
  if (facet_neighbour<TDIM>(conn, v2c_off, v2c, c, lf, nb, nlf) && inset[nb] && c < nb)
  {
    r = make_int4((int)c, lf, nb, nlf);
    atomicAdd(&counts[i], 1);
  }
  *reinterpret_cast<int4*>(cand + 4 * t) = r;
}

// ---------------------------------------------------------------------------
// 8f-4 facet hosts: cut(level_set, facets, tdim - 1) (cut.cpp:540-591, 788-830).  The hosts are facets of
// the mesh given as integration rows (cell, local facet[, cell1, local facet1]); host vertex j is either the
// j-th vertex of cell0 that is not opposite the facet (ascending local index) or the caller's
// entities_to_geometry row.  The sub-triangulation of a host is the (tdim-1)-dimensional marching case of its
// P1 level-set values; points live on the host's reference simplex, weights carry the physical measure.
// ---------------------------------------------------------------------------
template <int TDIM>
__global__ void __launch_bounds__(kBlock) facet_hosts_kernel(int64_t n, const int32_t* __restrict__ rows, int width,
                                                             const int32_t* __restrict__ geom,
                                                             const int32_t* __restrict__ conn, int64_t ncells,
                                                             const int32_t* __restrict__ ls_dofmap,
                                                             int32_t* __restrict__ verts, int32_t* __restrict__ ls, int* bad)
{
  constexpr int NV = TDIM + 1;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t c = rows[i * width];
  const int lf = rows[i * width + 1];
  if (c < 0 || c >= ncells || lf < 0 || lf > TDIM) { *bad = 1; return; }
  int32_t cv[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) cv[k] = conn[c * NV + k];
  for (int j = 0; j < TDIM; ++j)
  {
    int loc = -1;
    if (geom)
    {
      const int32_t g = geom[i * TDIM + j];
      for (int k = 0; k < NV; ++k) loc = (k != lf && cv[k] == g) ? k : loc;
    }
    else
      loc = j < lf ? j : j + 1;
    if (loc < 0) { *bad = 2; return; }
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) v = (k == loc) ? cv[k] : v;
    verts[i * TDIM + j] = v;
    ls[i * TDIM + j] = ls_dofmap[c * NV + loc];
  }
  if (width == 4)
  {
    const int64_t c1 = rows[i * 4 + 2];
    const int lf1 = rows[i * 4 + 3];
    if (c1 < 0 || c1 >= ncells || lf1 < 0 || lf1 > TDIM) { *bad = 1; return; }
    // the same facet seen from cell1: every facet vertex of cell0 is a vertex of cell1 other than lf1
    for (int k = 0; k < NV; ++k)
    {
      if (k == lf) continue;
      bool found = false;
      for (int m = 0; m < NV; ++m) found = found || (m != lf1 && conn[c1 * NV + m] == cv[k]);
      if (!found) { *bad = 3; return; }
    }
  }
}

__global__ void __launch_bounds__(kBlock) iota_kernel(int64_t n, int32_t* __restrict__ a)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) a[i] = (int32_t)i;
}

// exterior facets: per cell the bit mask of its local facets without a neighbour
template <int TDIM>
__global__ void __launch_bounds__(kBlock) exterior_mask_kernel(int64_t ncells, const int32_t* __restrict__ conn,
                                                               const int64_t* __restrict__ v2c_off,
                                                               const int32_t* __restrict__ v2c, uint8_t* __restrict__ mask)
{
  constexpr int NV = TDIM + 1;
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= ncells) return;
  unsigned m = 0;
  for (int lf = 0; lf < NV; ++lf)
  {
    int32_t nb;
    int nlf;
    if (!facet_neighbour<TDIM>(conn, v2c_off, v2c, c, lf, nb, nlf)) m |= 1u << lf;
  }
  mask[c] = (uint8_t)m;
}

__global__ void __launch_bounds__(kBlock) exterior_count_kernel(int64_t n, const int32_t* __restrict__ cells,
                                                                const uint8_t* __restrict__ mask, int32_t* __restrict__ counts)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) counts[i] = __popc((unsigned)mask[cells[i]]);
}

__global__ void __launch_bounds__(kBlock) exterior_pack_kernel(int64_t n, const int32_t* __restrict__ cells,
                                                               const uint8_t* __restrict__ mask,
                                                               const int64_t* __restrict__ offs, int32_t* __restrict__ rows)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t c = cells[i];
  unsigned m = mask[c];
  int64_t o = offs[i];
  for (int lf = 0; lf < 4; ++lf)
    if ((m >> lf) & 1u) { rows[2 * o] = c; rows[2 * o + 1] = lf; ++o; }
}

struct ByteSet
{
  const uint8_t* b;
  __device__ bool operator()(int64_t i) const { return b[i] != 0; }
};

struct IsCut
{
  const int8_t* domain;
  __device__ bool operator()(int64_t c) const { return domain[c] == CFX_INTERSECTED; }
};

// the per-tile counters of the first level set, zeroed: two arrays in one block
static void tile_counters(cfx_cut_t cut, int64_t ntiles, bool zeroed_already)
{
  const int64_t stride = (ntiles + 3) & ~3LL;
  if (!zeroed_already)
  {
    cut->tile_block.alloc(2 * stride);
    cut->tile_block.zero();
  }
  cut->tiles_inside.release(); cut->tiles_cut.release();
  cut->tiles_inside.p = cut->tile_block.p; cut->tiles_inside.n = ntiles; cut->tiles_inside.owned = false;
  cut->tiles_cut.p = cut->tile_block.p + stride; cut->tiles_cut.n = ntiles; cut->tiles_cut.owned = false;
}

void classify(cfx_cut_t cut)
{
  const int64_t nc = cut->nhosts();
  cut->block_class.release(); // (set again by the culled classification of level set 0)
  ++cut->gen;                 // the located lists of the previous classification lose their provenance
  provenance_forget_cut(cut);
  for (int k = 0; k < cut->nls; ++k)
  {
    int8_t* dom = cut->domain.p + (int64_t)k * nc;
    // (the codes of level set 0 stay with the cut: a row plan classifies row tiles from them)
    // ... next to one byte per level-set dof that the classification sets on the dofs of every cut cell: a dof with
    // a negative (positive) value and no cut cell around it has only inside (outside) cells around it)
    DevArray<uint8_t> codes_k;
    // (allocated in whole 16 B words: the block decision loads the words the last dofs lie in.  The pad bytes are never
    // written; no descriptor's mask names them, so they take no part in a block's decision.  A quarter's decision ANDs
    // whole words and may meet them: whatever they hold can only send a uniform quarter cell by cell, class_spans_and_words)
    const int64_t code_bytes = class_code_bytes(cut->ls_ndofs);
    if (k == 0 && cut->codes0.n != code_bytes) { cut->codes0.alloc(code_bytes); cut->touch0.alloc(cut->ls_ndofs); }
    if (k != 0) codes_k.alloc(code_bytes);
    struct { uint8_t* p; } codes{k == 0 ? cut->codes0.p : codes_k.p};
    uint8_t* touch = k == 0 ? cut->touch0.p : nullptr;
    if (k == 0) cut->touch_valid = false;
    // (the per-tile counters of level set 0 are cleared by the same launch when they fit its grid)
    bool tiles_zeroed = false;
    int32_t* zero_this = nullptr;
    int64_t zero_n = 0;
    if (k == 0 && cut->host_mask.n == 0)
    {
      const int64_t stride = (((nc + kByteTile - 1) / kByteTile) + 3) & ~3LL;
      if (2 * stride <= cut->ls_ndofs)
      {
        cut->tile_block.alloc(2 * stride);
        zero_this = cut->tile_block.p; zero_n = 2 * stride;
        tiles_zeroed = true;
      }
    }
    // (four values per thread when the level set starts on a 16 B boundary and the grid still covers the counters)
    const int64_t quads = (cut->ls_ndofs + 3) / 4;
    if ((reinterpret_cast<uintptr_t>(cut->ls_values[k].p) & 15) == 0 && (reinterpret_cast<uintptr_t>(codes.p) & 3) == 0
        && (reinterpret_cast<uintptr_t>(touch) & 3) == 0 && zero_n <= quads)
      launch("sign_codes", sign_codes4_kernel, grid_for(quads), dim3(kBlock), 0, cut->ls_ndofs, cut->ls_values[k].p, codes.p,
             zero_this, zero_n, touch);
    else
      launch("sign_codes", sign_codes_kernel, grid_for(cut->ls_ndofs), dim3(kBlock), 0, cut->ls_ndofs, cut->ls_values[k].p,
             codes.p, zero_this, zero_n, touch);
    const uint8_t* phi = codes.p;
    {
      // implicit-structured variant (opt-in): generated box mesh, P1 level set on the geometry dofmap
      cfx_mesh_t mesh = cut->mesh;
      if (env_is<Sw::IMPLICIT_BOX>('1') && cut->host_width == 0 && mesh->box_n > 0 && cut->ls_dofmap.p == mesh->conn.p
          && cut->ls_ndofs_cell == mesh->tdim + 1)
      {
        const int64_t ncubes = nc / (mesh->tdim == 3 ? 6 : 2);
        int32_t *b_in = nullptr, *b_cut = nullptr;
        if (k == 0 && cut->host_mask.n == 0)
        {
          const int64_t ntiles = (nc + kByteTile - 1) / kByteTile;
          tile_counters(cut, ntiles, tiles_zeroed);
          b_in = cut->tiles_inside.p; b_cut = cut->tiles_cut.p;
        }
        else if (k == 0) { cut->tiles_inside.release(); cut->tiles_cut.release(); }
        for_tdim(mesh->tdim, [&](auto T) {
          launch("classify_box", classify_box_kernel<T()>, grid_for(ncubes), dim3(kBlock), 0, ncubes, mesh->box_n, phi, dom,
                 b_in, b_cut, touch);
        });
        if (k == 0) cut->touch_valid = true;
        continue;
      }
    }
    int32_t *t_in = nullptr, *t_cut = nullptr;
    if (k == 0 && cut->host_mask.n == 0)
    {
      const int64_t ntiles = (nc + kByteTile - 1) / kByteTile;
      tile_counters(cut, ntiles, tiles_zeroed);
      t_in = cut->tiles_inside.p; t_cut = cut->tiles_cut.p;
    }
    else if (k == 0) { cut->tiles_inside.release(); cut->tiles_cut.release(); }
    {
      // block culling (classify_culled_kernel): cells as hosts, level set on the geometry dofmap (the summary is the
      // mesh's), P1; CFX_CLASSIFY_CULL=0: cell by cell
      cfx_mesh_t mesh = cut->mesh;
      const int nd = cut->ls_ndofs_cell;
      if (env_on<Sw::CLASSIFY_CULL>() && cut->host_width == 0 && cut->ls_dofmap.p == mesh->conn.p && nd == mesh->tdim + 1
          && nc == mesh->ncells && (nd == 3 || nd == 4))
      {
        const int64_t nb = (nc + kClassBlock - 1) / kClassBlock;
        if (!mesh->class_built)
        {
          mesh->class_nruns.alloc(nb);
          mesh->class_runs.alloc(nb * kClassRuns);
          mesh->class_sub_runs.alloc(nb * kClassSub * kClassSubRuns);
          if (nd == 4)
            launch("classify_summary", class_summary_kernel<4, kClassBlock, kClassRuns, 1024, 4096>, dim3((unsigned)nb), dim3(kBlock), 0,
                   nc, mesh->conn.p, mesh->class_nruns.p, mesh->class_runs.p, mesh->class_sub_runs.p);
          else
            launch("classify_summary", class_summary_kernel<3, kClassBlock, kClassRuns, 1024, 4096>, dim3((unsigned)nb), dim3(kBlock), 0,
                   nc, mesh->conn.p, mesh->class_nruns.p, mesh->class_runs.p, mesh->class_sub_runs.p);
          mesh->class_built = true;
          publish_across_lanes();
        }
        const dim3 cgrid((unsigned)(((nb + 1) / 2 + kBlock / 64 - 1) / (kBlock / 64)));   // a wavefront per pair of blocks
        uint8_t* bclass = nullptr;
        if (k == 0 && t_in != nullptr) { cut->block_class.alloc(nb); bclass = cut->block_class.p; }
        // the block decision from the mesh-static chunk descriptors (built at the first classification that takes them):
        // the sign codes are loaded as whole 16 B words, so they start on a 16 B boundary (their allocation covers
        // whole words: code_bytes above); CFX_CLASSIFY_CHUNKS=0: from the runs
        const bool chunked = env_on<Sw::CLASSIFY_CHUNKS>() && (reinterpret_cast<uintptr_t>(phi) & 15) == 0;
        if (chunked && mesh->class_chunks.n == 0)
        {
          const int64_t nbp = (nb + 1) & ~int64_t(1);
          mesh->class_chunks.alloc(nbp * kClassChunks);
          launch("classify_chunks", class_chunks_kernel, dim3((unsigned)((nbp + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                 nb, nbp, (const int2*)mesh->class_runs.p, mesh->class_chunks.p);
          publish_across_lanes();
        }
        const int2 *runs = mesh->class_runs.p, *chunks = mesh->class_chunks.p, *sub_runs = mesh->class_sub_runs.p;
        auto block_pass = [&](auto kernel) {
          launch("classify", kernel, cgrid, dim3(kBlock), 0, nc, nb, cut->ls_dofmap.p, runs, chunks, sub_runs, phi, dom, t_in, t_cut, bclass,
                 touch);
        };
        if (nd == 4 && chunked) block_pass(classify_culled_kernel<4, true>);
        else if (nd == 4) block_pass(classify_culled_kernel<4, false>);
        else if (chunked) block_pass(classify_culled_kernel<3, true>);
        else block_pass(classify_culled_kernel<3, false>);
        if (k == 0) cut->touch_valid = true;
        continue;
      }
    }
    switch (cut->ls_ndofs_cell)
    {
    case 2: launch("classify", classify_kernel<2>, grid_for(nc, kBlock * CFX_CLASSIFY_UNROLL), dim3(kBlock), 0, nc, cut->ls_dofmap.p, phi, dom, t_in, t_cut, touch); break;
    case 3: launch("classify", classify_kernel<3>, grid_for(nc, kBlock * CFX_CLASSIFY_UNROLL), dim3(kBlock), 0, nc, cut->ls_dofmap.p, phi, dom, t_in, t_cut, touch); break;
    case 4: launch("classify", classify_kernel<4>, grid_for(nc, kBlock * CFX_CLASSIFY_UNROLL), dim3(kBlock), 0, nc, cut->ls_dofmap.p, phi, dom, t_in, t_cut, touch); break;
    case 6: launch("classify", classify_kernel<6>, grid_for(nc, kBlock * CFX_CLASSIFY_UNROLL), dim3(kBlock), 0, nc, cut->ls_dofmap.p, phi, dom, t_in, t_cut, touch); break;
    case 10: launch("classify", classify_kernel<10>, grid_for(nc, kBlock * CFX_CLASSIFY_UNROLL), dim3(kBlock), 0, nc, cut->ls_dofmap.p, phi, dom, t_in, t_cut, touch); break;
    default: throw Error(CFX_ERR_INVALID_ARGUMENT, "unsupported level-set element (dofs per cell must be 3, 4, 6 or 10)");
    }
    if (k == 0) cut->touch_valid = true;
  }
  if (cut->host_mask.n > 0)
    for (int k = 0; k < cut->nls; ++k)
      launch("restrict_domain", restrict_domain_kernel, grid_for(nc), dim3(kBlock), 0, nc, cut->host_mask.p,
             cut->domain.p + (int64_t)k * nc);
  cut->located.clear();
  cut->located_ids.clear();
  cut->ghost_rows.clear();
}

__global__ void __launch_bounds__(kBlock) count_block_class_kernel(int64_t n, const uint8_t* __restrict__ block_class,
                                                                   unsigned long long* __restrict__ counts)
{
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned c = i < n ? (unsigned)block_class[i] : 0u;
  const unsigned long long inside = __ballot(c == 1u), outside = __ballot(c == 2u);
  if ((threadIdx.x & 63) == 0)
  {
    if (inside) atomicAdd(&counts[0], (unsigned long long)__popcll(inside));
    if (outside) atomicAdd(&counts[1], (unsigned long long)__popcll(outside));
  }
}

// "phi<0" and "phi=0" of the first level set in one pass over the classification bytes: every solve asks for
// both (the uncut entities, and the cut cells behind runtime_quadrature), and the classification has counted both
__global__ void __launch_bounds__(kBlock) locate_inside_cut_kernel(int64_t n, const uint8_t* __restrict__ bytes,
                                                                   const int64_t* __restrict__ off_in,
                                                                   const int64_t* __restrict__ off_cut,
                                                                   int32_t* __restrict__ out_in, int32_t* __restrict__ out_cut,
                                                                   DevN n_in_d, DevN n_cut_d, const uint8_t* __restrict__ block_class)
{
  // (lists sized by the previous step: nothing is written when a total did not fit -- dev_n is 0 in a void step)
  const int64_t n_in = dev_n(n_in_d), n_cut = dev_n(n_cut_d);
  const int64_t base = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kByteItems;
  unsigned f_in = 0, f_cut = 0;
  // what the culled classification knows about whole blocks of kClassBlock cells saves the bytes of the uniform ones:
  // a tile of outside blocks (two thirds of the 512^3 mesh) is left at once, an inside block lists its cells unread
  unsigned cls = 0;
  if (block_class)
  {
    constexpr int BPT = kByteTile / kClassBlock;
    const int64_t nblocks = (n + kClassBlock - 1) / kClassBlock;
    unsigned tile_all = 3u;
#pragma unroll
    for (int j = 0; j < BPT; ++j)
    {
      const int64_t bj = (int64_t)blockIdx.x * BPT + j;
      tile_all &= bj < nblocks ? (unsigned)block_class[bj] : 2u;
    }
    if (tile_all == 2u) return;
    cls = base < n ? (unsigned)block_class[base / kClassBlock] : 2u;
  }
  if (base < n && cls == 0u)
  {
    f_in = byte_flags(bytes, base, n, DomainMask{1});
    f_cut = byte_flags(bytes, base, n, DomainMask{2});
  }
  else if (base < n && cls == 1u)
    f_in = base + kByteItems <= n ? 0xffffu : ((1u << (int)(n - base)) - 1u);
  // the inside cells (the dense list) are packed in LDS and stored as one coalesced run per tile; the few cut
  // cells go out directly
  __shared__ int32_t s_in[kByteTile];
  int total_in, total;
  int o_in = block_exclusive_scan<int>(__popc(f_in), total_in);
  const int o_cut = block_exclusive_scan<int>(__popc(f_cut), total);
  int64_t b = off_cut[blockIdx.x] + o_cut;
#pragma unroll
  for (int k = 0; k < kByteItems; ++k)
  {
    if (f_in & (1u << k)) s_in[o_in++] = (int32_t)(base + k);
    if (f_cut & (1u << k)) { if (b < n_cut) out_cut[b] = (int32_t)(base + k); ++b; }
  }
  __syncthreads();
  const int64_t a = off_in[blockIdx.x];
  for (int i = threadIdx.x; i < total_in; i += kBlock)
    if (a + i < n_in) out_in[a + i] = s_in[i];
}

} // namespace

namespace cfx
{

const DevArray<int32_t>& locate(cfx_cut_t cut, const std::string& selector)
{
  auto it = cut->located.find(selector);
  if (it != cut->located.end()) return it->second;
  const int64_t nh = cut->nhosts();
  SelectorPred pred{cut->domain.p, nh, parse_selector(selector.c_str(), cut->nls)};
  DevArray<int32_t> out;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(cut->domain.p) + (int64_t)pred.sel.ls[0] * nh;
  if (pred.sel.n == 1 && (reinterpret_cast<uintptr_t>(bytes) & 15) == 0)
  {
    // "phi<0" / "phi=0" of the first level set: the classification already counted the tiles
    if (pred.sel.ls[0] == 0 && cut->tiles_inside.n > 0 && (pred.sel.mask[0] == 1 || pred.sel.mask[0] == 2)
        && cut->located.find("phi<0") == cut->located.end() && cut->located.find("phi=0") == cut->located.end()
        && (selector == "phi<0" || selector == "phi=0"))
    {
      const int64_t ntiles = cut->tiles_inside.n;
      DevArray<int64_t> off_in(ntiles + 1), off_cut(ntiles + 1);
      // (both totals in one round trip -- or none: inside a step they stay in HBM, published by the second scan, and
      // the lists are sized by the last step)
      const char* names[2] = {"locate.inside", "locate.cut"};
      const CountSource src[2] = {{off_in.p + ntiles, kCountI64, kCountUpTo}, {off_cut.p + ntiles, kCountI64, kCountUpTo}};
      CountPlan cp(2, names, src);
      exclusive_scan_pair(cut->tiles_inside.p, off_in.p, cut->tiles_cut.p, off_cut.p, ntiles, &cp);
      Count cnt[2];
      cp.finish(cnt);
      DevArray<int32_t> l_in(cnt[0].cap()), l_cut(cnt[1].cap());
      l_in.count = cnt[0]; l_cut.count = cnt[1];
      launch("locate_entities", locate_inside_cut_kernel, dim3((unsigned)ntiles), dim3(kBlock), 0, nh, bytes, off_in.p,
             off_cut.p, l_in.p, l_cut.p, l_in.devn(), l_cut.devn(),
             cut->block_class.n == (nh + kClassBlock - 1) / kClassBlock ? (const uint8_t*)cut->block_class.p : (const uint8_t*)nullptr);
      list_register(l_in.p, l_in.count);
      list_register(l_cut.p, l_cut.count);
      if (cut->host_width == 0 && cut->host_mask.n == 0) provenance_register(l_in.p, cut, cut->gen, -1, l_in.n);
      cut->located.emplace("phi<0", std::move(l_in));
      cut->located.emplace("phi=0", std::move(l_cut));
      return cut->located.find(selector)->second;
    }
    const int32_t* known = nullptr;
    if (pred.sel.ls[0] == 0 && cut->tiles_inside.n > 0)
      known = pred.sel.mask[0] == 1 ? cut->tiles_inside.p : (pred.sel.mask[0] == 2 ? cut->tiles_cut.p : nullptr);
    compact_bytes("locate_entities", nh, bytes, DomainMask{pred.sel.mask[0]}, out, known); // 1 B/cell stream
    // ("phi<0" / "phi>0" of level set 0 over all cells: the list is a function of the classification)
    if (pred.sel.ls[0] == 0 && cut->host_width == 0 && cut->host_mask.n == 0 && (pred.sel.mask[0] == 1 || pred.sel.mask[0] == 4))
      provenance_register(out.p, cut, cut->gen, pred.sel.mask[0] == 1 ? -1 : 1, out.n);
  }
  else
    compact("locate_entities", nh, pred, out);
  auto res = cut->located.emplace(selector, std::move(out));
  return res.first->second;
}

// the list with its exact length on the host (callers that size host-side work by it)
const DevArray<int32_t>& locate_exact(cfx_cut_t cut, const std::string& selector)
{
  DevArray<int32_t>& a = const_cast<DevArray<int32_t>&>(locate(cut, selector));
  if (a.count.cell)
  {
    a.n = a.count.value();
    list_unregister(a.p);
    a.count = Count();
  }
  return a;
}

void iota(int64_t n, int32_t* a) { launch("iota", iota_kernel, grid_for(n), dim3(kBlock), 0, n, a); }

} // namespace cfx

const cfx::DevArray<int32_t>& cfx_mesh_s::cell_neighbours()
{
  if (c2c_built) return c2c;
  const Adjacency& adj = vertex_cells();
  c2c.alloc(ncells * (int64_t)(tdim + 1));
  if (ncells > 0)
    for_tdim(tdim, [&](auto T) {
      launch("cell_neighbours", cell_neighbours_kernel<T(), true>, xcd_grid((ncells + kBlock - 1) / kBlock), dim3(kBlock), 0,
             ncells, conn.p, adj.offsets.p, adj.cells.p, c2c.p);
    });
  c2c_built = true;
  cfx::publish_across_lanes();
  return c2c;
}

extern "C" {

int cfx_cut_options_default(cfx_cut_options* opt)
{
  CFX_API_BEGIN
  require(opt != nullptr, CFX_ERR_INVALID_ARGUMENT, "null options");
  opt->cut_approximation_order = 1;
  opt->max_refinement_iterations = 8;
  opt->edge_max_depth = 20;
  opt->reserved = 0;
  CFX_API_END
}

int cfx_cut_create(cfx_mesh_t mesh, int nls, const int32_t* ls_dofmap, int ls_ndofs_cell, int64_t ls_ndofs,
                   const double* const* ls_values, const cfx_cut_options* opt, cfx_cut_t* out)
{
  CFX_API_BEGIN
  ctx().ensure();
  require(mesh && out, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create: null mesh/output");
  // cut.cpp:97-107: at least one level set
  require(nls >= 1 && ls_values, CFX_ERR_INVALID_ARGUMENT, "cutfemx.cut requires at least one level-set function");
  require(nls <= 8, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create: at most 8 level sets");
  require(ls_dofmap && ls_ndofs > 0, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create: empty level-set dofmap");
  ensure_cases();
  auto cut = std::make_unique<cfx_cut_s>();
  cut->mesh = mesh;
  cut->nls = nls;
  cut->ls_ndofs_cell = ls_ndofs_cell;
  cut->ls_ndofs = ls_ndofs;
  if (opt) cut->options = *opt; else cfx_cut_options_default(&cut->options);
  require(cut->options.cut_approximation_order == 1, CFX_ERR_INVALID_ARGUMENT,
          "cfx_cut_create: only straight (order-1) cut approximation is implemented");
  cut->ls_dofmap = to_device(ls_dofmap, mesh->ncells * (int64_t)ls_ndofs_cell);
  for (int k = 0; k < nls; ++k)
  {
    require(ls_values[k] != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create: null level-set values");
    cut->ls_values.push_back(to_device(ls_values[k], ls_ndofs));
  }
  cut->domain.alloc((int64_t)nls * mesh->ncells);
  classify(cut.get());
  *out = cut.release();
  CFX_API_END
}

int cfx_cut_restrict(cfx_cut_t cut, const int32_t* cells, int64_t n)
{
  CFX_API_BEGIN
  require(cut && (cells || n == 0) && n >= 0, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_restrict: null argument");
  require(cut->host_width == 0, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_restrict: the cut is hosted by facets (pass the subset to cfx_cut_create_facets)");
  const int64_t nc = cut->mesh->ncells;
  DevArray<int32_t> dcells = to_device(cells, n);
  cut->host_mask.alloc(nc);
  cut->host_mask.zero();
  ZeroFlag bad;
  launch("mark_subset", mark_subset_kernel, grid_for(n), dim3(kBlock), 0, n, dcells.p, nc, cut->host_mask.p, bad.p);
  require(!read_scalar(bad.p), CFX_ERR_OUT_OF_RANGE, "cfx_cut_restrict: cell index out of range");
  classify(cut);
  CFX_API_END
}

int cfx_cut_update(cfx_cut_t cut, const double* const* ls_values)
{
  CFX_API_BEGIN
  require(cut != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_update: null handle");
  if (ls_values)
    for (int k = 0; k < cut->nls; ++k)
      if (ls_values[k]) cut->ls_values[k] = to_device(ls_values[k], cut->ls_ndofs);
  classify(cut);
  CFX_API_END
}

int cfx_cut_info(cfx_cut_t cut, int* tdim, int* gdim, int64_t* ncells, int* nls)
{
  CFX_API_BEGIN
  require(cut != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_info: null handle");
  if (tdim) *tdim = cut->host_dim();
  if (gdim) *gdim = cut->mesh->gdim;
  if (ncells) *ncells = cut->nhosts();
  if (nls) *nls = cut->nls;
  CFX_API_END
}

int cfx_cut_domain(cfx_cut_t cut, int ls, const int8_t** domain)
{
  CFX_API_BEGIN
  require(cut && domain, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_domain: null argument");
  require(ls >= 0 && ls < cut->nls, CFX_ERR_OUT_OF_RANGE, "level-set index out of range");
  *domain = cut->domain.p + (int64_t)ls * cut->nhosts();
  CFX_API_END
}

int cfx_cut_uniform_blocks(cfx_cut_t cut, int64_t* n_inside, int64_t* n_outside)
{
  CFX_API_BEGIN
  require(cut && n_inside && n_outside, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_uniform_blocks: null argument");
  *n_inside = *n_outside = -1;
  const int64_t nb = cut->block_class.n;
  if (nb == 0) return CFX_OK;
  cfx::DevArray<unsigned long long> counts(2);
  counts.zero();
  cfx::launch("count_block_class", count_block_class_kernel, cfx::grid_for(nb), dim3(cfx::kBlock), 0, nb,
              (const uint8_t*)cut->block_class.p, counts.p);
  unsigned long long a = 0, b = 0;
  cfx::read_two(counts.p, counts.p + 1, a, b);
  *n_inside = (int64_t)a; *n_outside = (int64_t)b;
  CFX_API_END
}

int cfx_locate_entities(cfx_cut_t cut, const char* selector, const int32_t** entities, int64_t* n)
{
  CFX_API_BEGIN
  require(cut && selector && entities && n, CFX_ERR_INVALID_ARGUMENT, "cfx_locate_entities: null argument");
  if (cut->host_width != 0) (void)locate_exact(cut, selector);
  const DevArray<int32_t>& a = locate(cut, selector);
  if (cut->host_width != 0)
  {
    // host_parent_index (cut.cpp:352-359): facet hosts answer with the caller's facet ids
    auto it = cut->located_ids.find(selector);
    if (it == cut->located_ids.end())
    {
      DevArray<int32_t> ids(a.n);
      gather_rows("locate_entities", a.n, a.p, 1, cut->host_ids.p, ids.p);
      it = cut->located_ids.emplace(selector, std::move(ids)).first;
    }
    *entities = it->second.p;
    *n = it->second.n;
    return CFX_OK;
  }
  *entities = a.p;
  *n = a.count.cell ? a.count.cap() : a.n; // (a capacity while the step that made the list is open, cutfemx_amd.h)
  CFX_API_END
}

int cfx_ghost_penalty_facets(cfx_cut_t cut, const char* selector, const int32_t** rows, int64_t* n)
{
  CFX_API_BEGIN
  require(cut && selector && rows && n, CFX_ERR_INVALID_ARGUMENT, "cfx_ghost_penalty_facets: null argument");
  require(cut->host_width == 0, CFX_ERR_INVALID_ARGUMENT, "ghost_penalty_facets needs a cut hosted by the mesh cells");
  cfx_mesh_t mesh = cut->mesh;
  {
    auto it = cut->ghost_rows.find(selector);
    if (it != cut->ghost_rows.end())
    {
      *rows = it->second.p;
      *n = it->second.count.cell ? it->second.count.cap() : it->second.n / 4;
      return CFX_OK;
    }
  }
  SelectorPred pred{cut->domain.p, mesh->ncells, parse_selector(selector, cut->nls)};
  const DevArray<int32_t>& cutc = locate(cut, "phi=0");
  const DevN ncut_d = cutc.devn();
  const int64_t ncut = ncut_d.cap; // (capacity while the list's length is in HBM: the counts behind it stay zero)
  const DevArray<int32_t>& c2c = mesh->cell_neighbours();
  DevArray<int32_t> counts(ncut), cand(ncut * (int64_t)(mesh->tdim + 1) * 4);
  DevArray<int64_t> offs(ncut + 1);
  Count total(0);
  if (ncut > 0)
  {
    for_tdim(mesh->tdim, [&](auto T) {
      launch("ghost_facets_find", ghost_facets_find_kernel<T()>, grid_for(ncut), dim3(kBlock), 0, ncut_d, cutc.p,
             mesh->conn.p, c2c.p, cut->domain.p, pred, counts.p, cand.p);
    });
    const char* gname = "ghost_facets";
    const CountSource gsrc{offs.p + ncut, kCountI64, kCountUpTo};
    CountPlan cp(1, &gname, &gsrc);
    exclusive_scan(counts.p, offs.p, ncut, &cp);
    cp.finish(&total);
  }
  DevArray<int32_t>& grows = cut->ghost_rows[selector];
  grows.alloc(total.cap() * 4);
  if (total.cap() > 0)
  {
    // (a total beyond the capacity voids the step before this launch: ncut_d then reads 0 and nothing is written)
    for_tdim(mesh->tdim, [&](auto T) {
      launch("ghost_facets_pack", ghost_facets_pack_kernel<T()>, grid_for(ncut), dim3(kBlock), 0, ncut_d, cand.p, offs.p,
             grows.p);
    });
  }
  if (total.cell)
  {
    grows.count = total;
    list_register(grows.p, total);
  }
  *rows = grows.p;
  *n = total.cap();
  CFX_API_END
}

int cfx_interior_facets_for_cells(cfx_mesh_t mesh, const int32_t* cells, int64_t n, int32_t** rows, int64_t* n_rows)
{
  CFX_API_BEGIN
  require(mesh && (cells || n == 0) && rows && n_rows && n >= 0, CFX_ERR_INVALID_ARGUMENT,
          "cfx_interior_facets_for_cells: null argument");
  const int64_t nc = mesh->ncells;
  DevArray<int32_t> dcells = to_device(cells, n);
  DevArray<uint8_t> inset(nc);
  inset.zero();
  ZeroFlag bad;
  launch("mark_subset", mark_subset_kernel, grid_for(n), dim3(kBlock), 0, n, dcells.p, nc, inset.p, bad.p);
  require(!read_scalar(bad.p), CFX_ERR_OUT_OF_RANGE, "cfx_interior_facets_for_cells: cell index out of range");
  DevArray<int32_t> sorted; // ascending, duplicates removed
  const int64_t m = compact("interior_facets", nc, ByteSet{inset.p}, sorted);
  const int nv = mesh->tdim + 1;
  DevArray<int32_t> counts(m), cand(m * nv * 4);
  DevArray<int64_t> offs(m + 1);
  int64_t total = 0;
  const Adjacency& adj = mesh->vertex_cells();
  if (m > 0)
  {
    counts.zero();
    for_tdim(mesh->tdim, [&](auto T) {
      launch("interior_facets_find", interior_facets_find_kernel<T()>, grid_for(m * nv), dim3(kBlock), 0, m, sorted.p,
             mesh->conn.p, adj.offsets.p, adj.cells.p, inset.p, counts.p, cand.p);
    });
    exclusive_scan(counts.p, offs.p, m);
    total = read_scalar(offs.p + m);
  }
  int32_t* out = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * 4 * (size_t)(total > 0 ? total : 1)));
  if (total > 0)
    for_tdim(mesh->tdim, [&](auto T) {
      launch("ghost_facets_pack", ghost_facets_pack_kernel<T()>, grid_for(m), dim3(kBlock), 0, m, cand.p, offs.p, out);
    });
  *rows = out;
  *n_rows = total;
  CFX_API_END
}

int cfx_cell_aggregation_create(cfx_cut_t cut, const char* selector, double threshold, int root_policy,
                                int max_iterations, int allow_rootless, cfx_aggregation_t* out)
{
  CFX_API_BEGIN
  require(cut && selector && out, CFX_ERR_INVALID_ARGUMENT, "cfx_cell_aggregation_create: null argument");
  require(cut->host_width == 0, CFX_ERR_INVALID_ARGUMENT, "Cell aggregation requires cell-hosted cut data."); // cell_aggregation.cpp:114
  require(threshold >= 0.0 && threshold <= 1.0, CFX_ERR_INVALID_ARGUMENT, "Volume fraction threshold must be in [0, 1].");
  require(root_policy == 0 || root_policy == 1, CFX_ERR_INVALID_ARGUMENT,
          "Unknown root policy. Expected 'interior_only' or 'interior_or_well_cut'.");
  const Selector sel = parse_selector(selector, cut->nls);
  require(sel.n == 1 && (sel.mask[0] == 1 || sel.mask[0] == 4), CFX_ERR_INVALID_ARGUMENT,
          "CellAggregation v1 expects a strict single level-set selector such as 'phi < 0' or 'phi > 0'.");
  cfx_mesh_t mesh = cut->mesh;
  const int64_t nc = mesh->ncells;
  const int tdim = mesh->tdim;
  const int8_t selcode = sel.mask[0] == 1 ? (int8_t)CFX_INSIDE : (int8_t)CFX_OUTSIDE;
  const int8_t* domain = cut->domain.p + (int64_t)sel.ls[0] * nc;
  auto A = std::make_unique<cfx_aggregation_s>();
  A->ncells = nc;
  A->root_cell.alloc(nc); A->aggregate_id.alloc(nc); A->depth.alloc(nc); A->fraction.alloc(nc);
  A->fraction.zero();
  dev_fill(A->root_cell.p, 0xff, sizeof(int32_t) * (size_t)nc);
  dev_fill(A->aggregate_id.p, 0xff, sizeof(int32_t) * (size_t)nc);
  dev_fill(A->depth.p, 0xff, sizeof(int32_t) * (size_t)nc);
  {
    // volume fraction of the selected part: order-1 rules of the cut cells (weights sum to the part's measure)
    cfx_rules_t rules = nullptr;
    const int rc = cfx_runtime_quadrature(cut, selector, 1, "straight", &rules);
    if (rc != CFX_OK) throw Error(rc, cfx_last_error());
    std::unique_ptr<cfx_rules_s> guard(rules);
    const int64_t nrules = rules->nr.value();
    if (nrules > 0)
      for_tdim(tdim, [&](auto T) {
        launch("agg_fraction", agg_fraction_kernel<T()>, grid_for(nrules), dim3(kBlock), 0, nrules, rules->offsets.p,
               rules->parent_map.p, rules->weights.p, mesh->x.p, mesh->conn.p, A->fraction.p);
      });
    CFX_HIP(hipStreamSynchronize(ctx().stream)); // the rules die here
  }
  DevArray<int32_t> t(nc);
  DevArray<uint8_t> cls(nc);
  launch("agg_init", agg_init_kernel, grid_for(nc), dim3(kBlock), 0, nc, domain, selcode, root_policy, A->fraction.p,
         threshold, t.p, cls.p);
  const int64_t n_interior = compact("agg_lists", nc, ClsMask{cls.p, 1, 0}, A->interior);
  const int64_t n_cut = compact("agg_lists", nc, ClsMask{cls.p, 2, 0}, A->cut);
  compact("agg_lists", nc, ClsMask{cls.p, 3, 0}, A->active);
  const int64_t n_well = compact("agg_lists", nc, ClsMask{cls.p, 4, 0}, A->well);
  const int64_t n_ill = compact("agg_lists", nc, ClsMask{cls.p, 8, 0}, A->ill);
  (void)n_interior; (void)n_cut;
  launch("agg_roots", agg_roots_kernel, grid_for(n_well), dim3(kBlock), 0, n_well, A->well.p, A->root_cell.p,
         A->aggregate_id.p, A->depth.p);
  const Adjacency& adj = mesh->vertex_cells();
  ZeroFlag changed;
  DevArray<int32_t> parent(n_ill);
  if (n_ill > 0)
  {
    for (int64_t it = 0;; ++it)
    {
      require(it <= nc, CFX_ERR_RUNTIME, "cell aggregation: relaxation did not converge");
      changed.zero();
      for_tdim(tdim, [&](auto T) {
        launch("agg_relax", agg_relax_kernel<T()>, grid_for(n_ill), dim3(kBlock), 0, n_ill, A->ill.p, mesh->conn.p,
               adj.offsets.p, adj.cells.p, cls.p, t.p, changed.p);
      });
      if (!read_scalar(changed.p)) break;
    }
    const int64_t limit = max_iterations < 0 ? nc : max_iterations;
    for_tdim(tdim, [&](auto T) {
      launch("agg_parent", agg_parent_kernel<T()>, grid_for(n_ill), dim3(kBlock), 0, n_ill, A->ill.p, mesh->conn.p,
             adj.offsets.p, adj.cells.p, cls.p, t.p, limit, parent.p);
    });
    for (int64_t it = 0;; ++it)
    {
      require(it <= nc, CFX_ERR_RUNTIME, "cell aggregation: root propagation did not converge");
      changed.zero();
      launch("agg_resolve", agg_resolve_kernel, grid_for(n_ill), dim3(kBlock), 0, n_ill, A->ill.p, parent.p,
             A->root_cell.p, A->aggregate_id.p, A->depth.p, changed.p);
      if (!read_scalar(changed.p)) break;
    }
    launch("agg_flag_rootless", agg_flag_rootless_kernel, grid_for(n_ill), dim3(kBlock), 0, n_ill, A->ill.p,
           A->root_cell.p, cls.p);
  }
  const int64_t n_rootless = compact("agg_lists", nc, ClsMask{cls.p, 16, 0}, A->rootless);
  require(allow_rootless || n_rootless == 0, CFX_ERR_RUNTIME,
          "CellAggregation found active ill-posed cells without an admissible root. Adjust the root policy or "
          "threshold, or explicitly allow rootless aggregation for diagnostics.");
  DevArray<int32_t> bad;
  A->n_pairs = compact("agg_lists", nc, ClsMask{cls.p, 8, 16}, bad);
  A->pairs.alloc(A->n_pairs * 4);
  launch("agg_pairs", agg_pairs_kernel, grid_for(A->n_pairs), dim3(kBlock), 0, A->n_pairs, bad.p, A->root_cell.p,
         A->pairs.p);
  *out = A.release();
  CFX_API_END
}

int cfx_cell_aggregation_view_get(cfx_aggregation_t agg, cfx_aggregation_view* v)
{
  CFX_API_BEGIN
  require(agg && v, CFX_ERR_INVALID_ARGUMENT, "cfx_cell_aggregation_view_get: null argument");
  v->ncells = agg->ncells;
  v->root_cell = agg->root_cell.p; v->aggregate_id = agg->aggregate_id.p; v->propagation_depth = agg->depth.p;
  v->cut_volume_fraction = agg->fraction.p;
  v->active_cells = agg->active.p; v->n_active = agg->active.n;
  v->cut_cells = agg->cut.p; v->n_cut = agg->cut.n;
  v->interior_cells = agg->interior.p; v->n_interior = agg->interior.n;
  v->well_posed_cells = agg->well.p; v->n_well_posed = agg->well.n;
  v->ill_posed_cells = agg->ill.p; v->n_ill_posed = agg->ill.n;
  v->rootless_cells = agg->rootless.p; v->n_rootless = agg->rootless.n;
  v->pairs = agg->pairs.p; v->n_pairs = agg->n_pairs;
  CFX_API_END
}

int cfx_cell_aggregation_destroy(cfx_aggregation_t agg)
{
  CFX_API_BEGIN
  delete agg;
  CFX_API_END
}

int cfx_cut_destroy(cfx_cut_t cut)
{
  CFX_API_BEGIN
  delete cut;
  CFX_API_END
}

int cfx_exterior_facets(cfx_mesh_t mesh, int32_t** rows, int64_t* n_rows)
{
  CFX_API_BEGIN
  ctx().ensure();
  require(mesh && rows && n_rows, CFX_ERR_INVALID_ARGUMENT, "cfx_exterior_facets: null argument");
  const int64_t nc = mesh->ncells;
  const Adjacency& adj = mesh->vertex_cells();
  DevArray<uint8_t> mask(nc);
  for_tdim(mesh->tdim, [&](auto T) {
    launch("exterior_facets", exterior_mask_kernel<T()>, grid_for(nc), dim3(kBlock), 0, nc, mesh->conn.p, adj.offsets.p,
           adj.cells.p, mask.p);
  });
  DevArray<int32_t> cells;
  const int64_t m = compact("exterior_facets", nc, ByteSet{mask.p}, cells);
  DevArray<int32_t> counts(m);
  DevArray<int64_t> offs(m + 1);
  int64_t total = 0;
  if (m > 0)
  {
    launch("exterior_facets", exterior_count_kernel, grid_for(m), dim3(kBlock), 0, m, cells.p, mask.p, counts.p);
    exclusive_scan(counts.p, offs.p, m);
    total = read_scalar(offs.p + m);
  }
  int32_t* out = static_cast<int32_t*>(dev_alloc(sizeof(int32_t) * 2 * (size_t)(total > 0 ? total : 1)));
  if (total > 0)
    launch("exterior_facets", exterior_pack_kernel, grid_for(m), dim3(kBlock), 0, m, cells.p, mask.p, offs.p, out);
  CFX_HIP(hipStreamSynchronize(ctx().stream));
  *rows = out;
  *n_rows = total;
  CFX_API_END
}

int cfx_cut_create_facets(cfx_mesh_t mesh, int64_t n, const int32_t* facet_ids, const int32_t* rows, int row_width,
                          const int32_t* entity_geometry, int nls, const int32_t* ls_dofmap, int ls_ndofs_cell,
                          int64_t ls_ndofs, const double* const* ls_values, const cfx_cut_options* opt, cfx_cut_t* out)
{
  CFX_API_BEGIN
  ctx().ensure();
  require(mesh && out, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: null mesh/output");
  require(n >= 0 && (rows || n == 0), CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: null facet rows");
  require(row_width == 2 || row_width == 4, CFX_ERR_INVALID_ARGUMENT,
          "cfx_cut_create_facets: rows are (cell, local facet) or (cell0, local facet0, cell1, local facet1)");
  require(nls >= 1 && ls_values, CFX_ERR_INVALID_ARGUMENT, "cutfemx.cut requires at least one level-set function");
  require(nls <= 8, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: at most 8 level sets");
  require(ls_dofmap && ls_ndofs > 0, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: empty level-set dofmap");
  const int tdim = mesh->tdim;
  require(ls_ndofs_cell == tdim + 1, CFX_ERR_INVALID_ARGUMENT,
          "cfx_cut_create_facets: facet hosts take a P1 level set (its dofs on a facet are its vertex dofs)");
  ensure_cases();
  auto cut = std::make_unique<cfx_cut_s>();
  cut->mesh = mesh;
  cut->nls = nls;
  cut->ls_ndofs_cell = tdim; // dofs per host
  cut->ls_ndofs = ls_ndofs;
  if (opt) cut->options = *opt; else cfx_cut_options_default(&cut->options);
  require(cut->options.cut_approximation_order == 1, CFX_ERR_INVALID_ARGUMENT,
          "cfx_cut_create_facets: only straight (order-1) cut approximation is implemented");
  cut->host_width = row_width;
  cut->n_hosts = n;
  cut->host_rows.alloc(n * row_width);
  cut->host_ids.alloc(n);
  cut->host_verts.alloc(n * tdim);
  cut->ls_dofmap.alloc(n * tdim);
  {
    DevArray<int32_t> drows = to_device(rows, n * row_width);
    DevArray<int32_t> dgeom = to_device(entity_geometry, entity_geometry ? n * tdim : 0);
    DevArray<int32_t> dls = to_device(ls_dofmap, mesh->ncells * (int64_t)ls_ndofs_cell);
    ZeroFlag bad;
    if (n > 0)
    {
      CFX_HIP(hipMemcpyAsync(cut->host_rows.p, drows.p, sizeof(int32_t) * (size_t)(n * row_width), hipMemcpyDeviceToDevice,
                             ctx().stream));
      if (facet_ids)
      {
        DevArray<int32_t> dids = to_device(facet_ids, n);
        CFX_HIP(hipMemcpyAsync(cut->host_ids.p, dids.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, ctx().stream));
        CFX_HIP(hipStreamSynchronize(ctx().stream));
      }
      else
        iota(n, cut->host_ids.p);
      const int32_t* geom = entity_geometry ? dgeom.p : nullptr;
      for_tdim(tdim, [&](auto T) {
        launch("facet_hosts", facet_hosts_kernel<T()>, grid_for(n), dim3(kBlock), 0, n, drows.p, row_width, geom, mesh->conn.p,
               mesh->ncells, dls.p, cut->host_verts.p, cut->ls_dofmap.p, bad.p);
      });
    }
    const int b = read_scalar(bad.p);
    require(b != 1, CFX_ERR_OUT_OF_RANGE, "cfx_cut_create_facets: cell index or local facet out of range");
    require(b != 2, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: entity_geometry names a vertex that is not on the facet");
    require(b != 3, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: the two (cell, local facet) pairs of a row are different facets");
  }
  for (int k = 0; k < nls; ++k)
  {
    require(ls_values[k] != nullptr, CFX_ERR_INVALID_ARGUMENT, "cfx_cut_create_facets: null level-set values");
    cut->ls_values.push_back(to_device(ls_values[k], ls_ndofs));
  }
  cut->domain.alloc((int64_t)nls * n);
  classify(cut.get());
  *out = cut.release();
  CFX_API_END
}

} // extern "C"
