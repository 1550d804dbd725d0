// cutfemx_amd: the engine's environment switches -- ONE list, the only place in csrc/ that calls getenv.
//
// A switch is CFX_<NAME> in the environment and Sw::<NAME> in the code.  Every line of the list gives
//   kind  first_char: the first character of the value decides ('0' switches a default off, '1' an opt-in on, ...)
//         present:    being set at all is what counts
//         integer:    a number; the default is the reading site's argument and stands in the effect text
//         string:     compared whole
//   when  call:  read on every call that consults it -- setting or unsetting it in a running process takes effect
//         build: read when a mesh-static table of a space is built (the table then keeps what it was built as)
//         once:  read the first time it is consulted and cached for the life of the process
// and a one-line effect (DESIGN.md section 8 has the same rows; tests/test_switches.py keeps the two in step).
// The accessors below check kind and timing at compile time and cost one getenv (call, build) or one guarded load (once).
#pragma once

#include <cstdlib>
#include <cstring>

// clang-format off
#define CFX_SWITCHES(CFX_SWITCH)                                                                                                   \
  CFX_SWITCH(DETERMINISTIC,      first_char, call,  "1: lane-ordered LDS accumulation instead of LDS atomics: bitwise reproducible matrices") \
  CFX_SWITCH(ASSEMBLY,           string,     call,  "atomic: the entity-parallel FP64-atomic kernels instead of the row gather") \
  CFX_SWITCH(STENCIL,            first_char, build, "0: no mesh-static row stencil (P1): hashed sparsity, searching gather") \
  CFX_SWITCH(STENCIL_LISTS,      first_char, build, "0: no neighbour lists for the other spaces (degree 2, vector-valued, DG)") \
  CFX_SWITCH(STENCIL_STAGED,     first_char, build, "0: two-pass stencil rows and tiles, the build a card short of memory takes (so does a tile whose union outgrows its staging row; tests reach both through this switch alone)") \
  CFX_SWITCH(TILES,              first_char, build, "0: no row tiles") \
  CFX_SWITCH(LATTICE_ROWS,       first_char, build, "0: no lattice flags and no template: every plain row is computed by the tile kernel") \
  CFX_SWITCH(LATTICE_SOURCE,     first_char, call,  "0: the P1 series source term of the lattice rows hex by hex instead of its closed form per row") \
  CFX_SWITCH(LATTICE_PATTERN,    first_char, call,  "0: plain rows' columns always copied from the stencil; 2: from the offset row whatever the number of plain rows") \
  CFX_SWITCH(P2_PLAIN,           first_char, build, "0: degree 2 without the slot-record kernel") \
  CFX_SWITCH(P2_CLOSED,          first_char, call,  "0: degree 2 stages uncut tensors instead of closed-form rows") \
  CFX_SWITCH(P2_MOMENTS,         first_char, call,  "0: degree 2 stages cut-cell stiffness tensors instead of moments") \
  CFX_SWITCH(P2_CUT_TENSORS,     first_char, call,  "0: per-integral rule tensors and moments instead of one tensor per cut cell") \
  CFX_SWITCH(P2_INTERFACE,       first_char, call,  "0: the general gather kernel for the degree-2 interface rows") \
  CFX_SWITCH(FACET_FOLD_STAGE1,  first_char, call,  "0: full facet tensors staged, folded in the gather; 2: folded tensors but no rank-one records") \
  CFX_SWITCH(BLOCK_PLAIN,        first_char, call,  "0: vector spaces without the dof-at-a-time kernel") \
  CFX_SWITCH(BLOCK_GATHER,       first_char, call,  "0: block spaces by the entity-parallel kernels instead of the block gather") \
  CFX_SWITCH(ROWS_SPLIT,         first_char, call,  "1: split plain / interface rows whatever their share (small meshes of the kernel-path tests)") \
  CFX_SWITCH(VEC_BLOCKS,         first_char, call,  "0 / 2: linear forms never / always by cell block (also read when a space builds its cell blocks)") \
  CFX_SWITCH(VEC_ROWORDER,       first_char, call,  "0: the P1 series source term without the row-ordered staging") \
  CFX_SWITCH(SOURCE_SERIES,      first_char, call,  "0: the P1 source term by quadrature instead of its series") \
  CFX_SWITCH(SOURCE_GROUPS,      first_char, call,  "0: the P1 series source term cell by cell instead of one hex per lane") \
  CFX_SWITCH(SOURCE_SHELL,       first_char, call,  "0: the hex kernel of the closed-form source term sifts every hex of the entity list instead of taking the shell hexes from the rows that read them; 2: shell hexes whatever the length of the list (default: from 4 M entities)") \
  CFX_SWITCH(STAGING_NAN,        first_char, call,  "1 (tests): the hex-corner planes of the staging start as NaN, the column indices of a new pattern as -1") \
  CFX_SWITCH(PLAIN_STAGE,        first_char, call,  "0: plain rows without LDS staging, the form that meshes with stencils longer than 32 take by themselves") \
  CFX_SWITCH(MFMA,               first_char, call,  "0: generic rows instead of the MFMA kernel for staged elasticity tensors") \
  CFX_SWITCH(CUT_TENSORS_P1,     first_char, call,  "0: the generic tensors of cut P1 cells") \
  CFX_SWITCH(P1_CUT_COMBINE,     first_char, call,  "0: one staged tensor per rule and integral of a degree-1 bilinear form instead of one per cut cell") \
  CFX_SWITCH(RECT_GATHER,        first_char, call,  "0: rectangular blocks by the entity-parallel atomic kernel") \
  CFX_SWITCH(BULK_ROWS,          first_char, call,  "0: row plans take their marks from the entity lists, not from the classification") \
  CFX_SWITCH(PATTERN_REUSE,      first_char, call,  "0: never copy rows from the space's previous pattern") \
  CFX_SWITCH(IMPLICIT_BOX,       first_char, call,  "1: classification of generated box meshes from the cube index") \
  CFX_SWITCH(CLASSIFY_CULL,      first_char, call,  "0: classification cell by cell instead of block culling") \
  CFX_SWITCH(CLASSIFY_CHUNKS,    first_char, call,  "0: the block and quarter decisions of the culled classification decode the vertex runs instead of loading whole 16 B words of sign codes (chunk descriptors)") \
  CFX_SWITCH(STEP_SPECULATE,     first_char, call,  "0: steps publish nothing, every size is read back where it is produced") \
  CFX_SWITCH(FUSED_TILES,        integer,    once,  "n: count + offsets + write of a sync-free step as one chained launch up to n tiles (default 512; 0: three launches)") \
  CFX_SWITCH(SCAN_CHAINED_TILES, integer,    once,  "n: scans up to n tiles in one chained launch (default 8192), longer ones in three") \
  CFX_SWITCH(COUNT_SYNC,         first_char, once,  "1: count the size read-backs; 2: also name each by the launch before it") \
  CFX_SWITCH(STEP_DEBUG,         present,    once,  "trace the sites of a step, their capacities and what voided it") \
  CFX_SWITCH(PLAN_DEBUG,         present,    call,  "print row-class counts of plans and patterns") \
  CFX_SWITCH(LAUNCH_TRACE,       present,    once,  "every kernel launch (name, grid) on stderr") \
  CFX_SWITCH(LAUNCH_SYNC,        present,    once,  "a stream synchronisation behind every launch: a fault surfaces at its own kernel") \
  CFX_SWITCH(ALLOC_TRACE,        present,    once,  "every hipMalloc of the block cache with its duration")
// clang-format on

namespace cfx
{

enum class Sw : int
{
#define CFX_SWITCH(NAME, kind, when, effect) NAME,
  CFX_SWITCHES(CFX_SWITCH)
#undef CFX_SWITCH
};

namespace sw
{
enum Kind { first_char, present, integer, string };
enum When { call, build, once };
struct Entry { const char* name; Kind kind; When when; };
constexpr Entry kTable[] = {
#define CFX_SWITCH(NAME, kind, when, effect) {"CFX_" #NAME, kind, when},
  CFX_SWITCHES(CFX_SWITCH)
#undef CFX_SWITCH
};
template <Sw S, Kind K, bool Cached>
inline const char* raw()
{
  constexpr Entry e = kTable[(int)S];
  static_assert(e.kind == K, "switch read as another kind than the table gives it");
  static_assert((e.when == once) == Cached, "switch read at another time than the table gives it");
  return getenv(e.name);
}
} // namespace sw

// --- read where they stand (when = call, build) ---
template <Sw S> inline char env_char() { const char* e = sw::raw<S, sw::first_char, false>(); return e ? e[0] : '\0'; } // three-way switches
template <Sw S> inline bool env_is(char c) { return env_char<S>() == c; } // set and first character == c (c != 0)
template <Sw S> inline bool env_on() { return !env_is<S>('0'); }          // not switched off
template <Sw S> inline bool env_present() { return sw::raw<S, sw::present, false>() != nullptr; }
template <Sw S> inline bool env_equals(const char* v) { const char* e = sw::raw<S, sw::string, false>(); return e && strcmp(e, v) == 0; }

// --- cached at the first reading (when = once): one value per process, whatever the number of reading sites ---
template <Sw S> inline char env_char_once() { static const char c = []() { const char* e = sw::raw<S, sw::first_char, true>(); return e ? e[0] : '\0'; }(); return c; }
template <Sw S> inline bool env_present_once() { static const bool on = sw::raw<S, sw::present, true>() != nullptr; return on; }
template <Sw S> inline long long env_int_once(long long dflt) { static const long long v = [&]() { const char* e = sw::raw<S, sw::integer, true>(); return e ? atoll(e) : dflt; }(); return v; }

} // namespace cfx
