// cutfemx_amd: the distance stage of the reinitialisation (cfx_reinit.hip) for the stages that build on it
// (cfx_extend.hip): the iteration run to its end with the distance left in a workspace, and the signed result written
// to any array.  cfx_reinitialize is the two in a row on phi itself.
#pragma once

#include "cfx_common.h"

namespace cfx
{
namespace reinit
{
struct ReinitRecord
{
  cfx_reinit_info info;        // what the caller receives (copied out as it stands)
  unsigned long long count[2]; // sweep s walks list s & 1 of count[s & 1] targets and fills the other one
};

// the workspace of one call, from the block cache
struct DistanceStage
{
  DevArray<double> d;          // [nv] the distance (inf_value: never reached); not clamped to the band
  DevArray<double> d0;         // [nv] the near field (only with keep_near)
  DevArray<double> cand;       // [nv] free once the iteration has ended, like the lists
  DevArray<int32_t> list0, list1;
  DevArray<unsigned> bits;
  DevArray<ReinitRecord> rec;
  double inf = 0.0, band = 0.0; // band <= 0: none
  int slot = 0;                // the list the last launched sweep filled (empty: converged)
};

// the argument checks of cfx_reinitialize, with the caller's name in the messages
void check_arguments(const char* who, cfx_space_t V, const cfx_reinit_options& o);
// begin, seed, start and the sweeps on the device array phi (read only)
void distance_stage(cfx_space_t V, const double* phi, const cfx_reinit_options& o, bool keep_near, DistanceStage& S);
// out = s min(d, B) and the reason in S.rec (out may be phi itself, or null: the reason alone); nothing is written without
// an interface
void write_signed_distance(cfx_space_t V, const DistanceStage& S, const double* phi, double* out);
} // namespace reinit
} // namespace cfx
