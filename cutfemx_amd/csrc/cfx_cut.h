// cutfemx_amd: what the classification (cfx_cut.hip) and the rules built on it (cfx_rules.hip) share.
#pragma once

#include <string>

#include "cfx_common.h"

namespace cfx
{

// ---------------------------------------------------------------------------
// selector: DNF over (level set, relation) clauses.  relation -> set of
// domains, cut.cpp:323-342.  bit0 inside, bit1 intersected, bit2 outside.
// ---------------------------------------------------------------------------
constexpr int kMaxClauses = 16;

struct Selector
{
  int n = 0;
  int ls[kMaxClauses];
  int mask[kMaxClauses];
  int term[kMaxClauses];
};

Selector parse_selector(const char* s, int nls); // cfx_cut.hip

struct SelectorPred
{
  const int8_t* domain;
  int64_t ncells;
  Selector sel;
  __device__ bool operator()(int64_t c) const
  {
    const int nterm = sel.term[sel.n - 1] + 1;
    for (int t = 0; t < nterm; ++t)
    {
      bool ok = true, any = false;
      for (int k = 0; k < sel.n; ++k)
      {
        if (sel.term[k] != t) continue;
        any = true;
        const int d = domain[(int64_t)sel.ls[k] * ncells + c];
        if (!((sel.mask[k] >> (d + 1)) & 1)) { ok = false; break; }
      }
      if (any && ok) return true;
    }
    return false;
  }
};

// the part of a cut host that a one-clause selector with a "<", "=" or ">" relation names
enum Part { PART_IN = 0, PART_OUT = 1, PART_IF = 2 };
inline int part_of_mask(int m) { return (m == 2) ? PART_IF : ((m & 1) ? PART_IN : PART_OUT); }

// the hosts a selector names, ascending (cached with the cut); _exact: with the list's length on the host
const DevArray<int32_t>& locate(cfx_cut_t cut, const std::string& selector);       // cfx_cut.hip
const DevArray<int32_t>& locate_exact(cfx_cut_t cut, const std::string& selector); // cfx_cut.hip

void iota(int64_t n, int32_t* a); // a[i] = i (cfx_cut.hip)

void ensure_cases(); // the sub-triangulation tables in constant memory, uploaded once (cfx_rules.hip)
// dst[i * width + k] = src[idx[i] * width + k] (cfx_rules.hip)
void gather_rows(const char* name, int64_t n, const int32_t* idx, int width, const int32_t* src, int32_t* dst);

} // namespace cfx
