// cutfemx_amd: functionals -- rank-0 forms assembled in HBM and returned as one double.
//
// Replaces cpp/dolfinx_custom_data/fem/assemble_scalar_impl.h:26-275 (python/cutfemx/fem.py assemble_scalar): the loop
// over the entities of every integral that adds the integrand's value to one scalar -- the L2 error, jump error,
// perimeter and compliance lines at the end of the reference's demos.
//
// Two launches per call.  functional_cells_kernel (or the rank-0 ending of a registered integrand's wrapper, cfx_rtc.hip):
// one thread per entity, 256 per block; a thread whose entity is a runtime rule loops over the rule's points; the
// thread's value is summed in FP64, the block's 256 values by a wave64 sum (__shfl_down) and the four wave sums through
// LDS, both in a fixed order, and the block stores ONE partial.  All integrals of the form write into one slab of partials
// at consecutive offsets.  functional_reduce_kernel: a single block adds the slab in a fixed order and stores the result.
// No floating-point atomics (the library is built with -munsafe-fp-atomics: their order is not fixed) and no hand-off
// between workgroups inside a launch: the launch boundary is the combine.  Two calls on the same inputs give the same
// bits.  Lengths are DevN: the grid comes from the capacity, a lane past the published length adds 0, and EVERY launched
// block stores its partial -- the slab is never zeroed.
#include "cfx_elem.h"

using namespace cfx;

namespace
{
enum { kFnField = 0, kFnL2Diff = 1, kFnH1Semi = 2 };

struct FnArgs
{
  const double* x;
  const int32_t* conn;
  const int32_t* dofmap;
  DevN n;                  // entities in this launch (length in HBM inside a sync-free step)
  const int32_t* entities; // standard cells
  const int32_t* offsets;  // runtime rules
  const int32_t* parent_map;
  const double* points;
  const double* weights;
  int qdegree;
  double params[8];
  const double* coeff;     // dof values of u_h ([ndofs][BS]), or null
  double* partials;        // one per block of this launch
};

// the sum of the block's 256 values in a fixed order, valid in thread 0.  Every thread of the block must arrive.
__device__ __forceinline__ double block_sum_fixed(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __shared__ double wave_sums[kBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);
}

// KIND: CFX_M_FIELD / CFX_M_L2_DIFF / CFX_M_H1_SEMI.  RT: the entity integrates over its runtime rule slice (weights
// are physical); otherwise over the reference rule of degree qdegree times |det J|.
template <int TDIM, int DEG, int BS, int KIND, bool RT>
__global__ void __launch_bounds__(kBlock) functional_cells_kernel(FnArgs A)
{
  constexpr int ND = Elem<TDIM, DEG>::ND;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double value = 0.0;
  if (e < dev_n(A.n)) // (a predicate, not a return: the block sum below has a barrier)
  {
    const int64_t cell = RT ? A.parent_map[e] : A.entities[e];
    Geo<TDIM> g;
    load_cell<TDIM>(A.x, A.conn, cell, g);
    jacobian<TDIM>(g);
    int npts;
    const double* pts;
    const double* wts;
    double wscale = 1.0;
    if constexpr (RT)
    {
      const int32_t q0 = A.offsets[e], q1 = A.offsets[e + 1];
      npts = q1 - q0;
      pts = A.points + (int64_t)q0 * TDIM;
      wts = A.weights + q0;
    }
    else
    {
      pts = ref_rule(TDIM, A.qdegree, npts, wts);
      wscale = fabs(g.detJ);
    }
    double cw[ND * BS];
#pragma unroll
    for (int j = 0; j < ND * BS; ++j) cw[j] = 0.0;
    if (A.coeff)
    {
      const int32_t* cd = A.dofmap + cell * ND;
#pragma unroll
      for (int j = 0; j < ND; ++j)
#pragma unroll
        for (int b = 0; b < BS; ++b) cw[j * BS + b] = A.coeff[(int64_t)cd[j] * BS + b];
    }
    const int field = (int)A.params[0];
    const double gscale = KIND == kFnL2Diff ? A.params[2] : 0.0;
    const bool analytic = KIND == kFnField ? field != CFX_F_COEFFICIENT : (KIND == kFnL2Diff && gscale != 0.0);
    double acc = 0.0;
    for (int q = 0; q < npts; ++q)
    {
      double X[TDIM];
#pragma unroll
      for (int t = 0; t < TDIM; ++t) X[t] = pts[(int64_t)q * TDIM + t];
      const double w = wts[q] * wscale;
      double f = 0.0; // the analytic field at the physical point
      if (analytic)
      {
        double xq[TDIM], l0 = 1.0;
#pragma unroll
        for (int t = 0; t < TDIM; ++t) l0 -= X[t];
#pragma unroll
        for (int d = 0; d < TDIM; ++d)
        {
          double v = l0 * g.x[0][d];
#pragma unroll
          for (int t = 0; t < TDIM; ++t) v += X[t] * g.x[t + 1][d];
          xq[d] = v;
        }
        f = field_eval<TDIM>(field, xq);
      }
      if constexpr (KIND == kFnH1Semi)
      {
        double N[ND], dN[ND][TDIM];
        tabulate<TDIM, DEG>(X, N, dN);
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < BS; ++b)
        {
          double gr[TDIM];
#pragma unroll
          for (int t = 0; t < TDIM; ++t)
          {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < ND; ++j) v += dN[j][t] * cw[j * BS + b];
            gr[t] = v;
          }
#pragma unroll
          for (int d = 0; d < TDIM; ++d)
          {
            double v = 0.0;
#pragma unroll
            for (int t = 0; t < TDIM; ++t) v += g.K[t][d] * gr[t];
            s += v * v;
          }
        }
        acc += w * s;
      }
      else
      {
        double N[ND];
        tabulate_values<TDIM, DEG>(X, N);
        if constexpr (KIND == kFnField)
        {
          if (!analytic)
          {
#pragma unroll
            for (int j = 0; j < ND; ++j) f += N[j] * cw[j * BS];
          }
          acc += w * f;
        }
        else
        {
          double s = 0.0;
#pragma unroll
          for (int b = 0; b < BS; ++b)
          {
            double u = 0.0;
#pragma unroll
            for (int j = 0; j < ND; ++j) u += N[j] * cw[j * BS + b];
            if (b == 0) u -= gscale * f;
            s += u * u;
          }
          acc += w * s;
        }
      }
    }
    value = A.params[1] * acc;
  }
  const double total = block_sum_fixed(value);
  if (threadIdx.x == 0) A.partials[blockIdx.x] = total;
}

// the second launch: ONE block adds the n partials in a fixed order (four strided running sums per thread, then the
// block sum) and OVERWRITES *out; n = 0 stores 0
__global__ void __launch_bounds__(kBlock) functional_reduce_kernel(const double* __restrict__ partials, int64_t n,
                                                                  double* __restrict__ out)
{
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int64_t i = threadIdx.x;
  for (; i + 3 * kBlock < n; i += 4 * kBlock)
  {
    a0 += partials[i];
    a1 += partials[i + kBlock];
    a2 += partials[i + 2 * kBlock];
    a3 += partials[i + 3 * kBlock];
  }
  for (; i < n; i += kBlock) a0 += partials[i];
  const double total = block_sum_fixed((a0 + a1) + (a2 + a3));
  if (threadIdx.x == 0) *out = total;
}

template <int TDIM, int DEG, int BS, int KIND>
void launch_cells_k(const FnArgs& A, bool runtime)
{
  const dim3 grid = grid_for(A.n.cap, kBlock);
  if (runtime)
    launch("functional_cells", functional_cells_kernel<TDIM, DEG, BS, KIND, true>, grid, dim3(kBlock), 0, A);
  else
    launch("functional_cells", functional_cells_kernel<TDIM, DEG, BS, KIND, false>, grid, dim3(kBlock), 0, A);
}

template <int TDIM, int DEG, int BS>
void launch_cells_t(int kernel, const FnArgs& A, bool runtime)
{
  switch (kernel)
  {
  case CFX_M_L2_DIFF: launch_cells_k<TDIM, DEG, BS, kFnL2Diff>(A, runtime); break;
  case CFX_M_H1_SEMI: launch_cells_k<TDIM, DEG, BS, kFnH1Semi>(A, runtime); break;
  default:
    // CFX_M_FIELD reads u_h on scalar spaces only (form creation checks it): one instantiation per element
    if constexpr (BS == 1) launch_cells_k<TDIM, DEG, 1, kFnField>(A, runtime);
    break;
  }
}

void launch_cells(const cfx_space_s* V, int kernel, const FnArgs& A, bool runtime)
{
  // (CFX_M_FIELD of an analytic field on a vector space: the element alone matters)
  const int bs = kernel == CFX_M_FIELD ? 1 : V->bs;
  const int key = V->mesh->tdim * 100 + V->degree * 10 + bs;
  switch (key)
  {
  case 211: launch_cells_t<2, 1, 1>(kernel, A, runtime); break;
  case 212: launch_cells_t<2, 1, 2>(kernel, A, runtime); break;
  case 213: launch_cells_t<2, 1, 3>(kernel, A, runtime); break;
  case 221: launch_cells_t<2, 2, 1>(kernel, A, runtime); break;
  case 222: launch_cells_t<2, 2, 2>(kernel, A, runtime); break;
  case 223: launch_cells_t<2, 2, 3>(kernel, A, runtime); break;
  case 311: launch_cells_t<3, 1, 1>(kernel, A, runtime); break;
  case 312: launch_cells_t<3, 1, 2>(kernel, A, runtime); break;
  case 313: launch_cells_t<3, 1, 3>(kernel, A, runtime); break;
  case 321: launch_cells_t<3, 2, 1>(kernel, A, runtime); break;
  case 322: launch_cells_t<3, 2, 2>(kernel, A, runtime); break;
  case 323: launch_cells_t<3, 2, 3>(kernel, A, runtime); break;
  default: throw Error(CFX_ERR_INVALID_ARGUMENT, "functionals: unsupported (tdim, degree, block size) combination");
  }
}

int64_t blocks_of(int64_t n) { return (n + kBlock - 1) / kBlock; }

// partials a call over ALL entities of integral I writes (sized from the capacities; the launches below write exactly
// these, in this order: standard entities, then runtime rules)
int64_t integral_blocks(const cfx_integral_dev& I)
{
  if (I.type == CFX_INTERIOR_FACET)
  {
    if (!(I.rules && I.n_std >= 0)) return blocks_of(I.n_entities.cap());
    const int64_t n = I.n_entities.value(); // (exact: form creation refuses a pending list next to facet-hosted rules)
    return blocks_of(std::min(I.n_std, n)) + blocks_of(n - std::min(I.n_std, n));
  }
  return blocks_of(I.n_entities.cap()) + (I.rules ? blocks_of(I.rules->nr.cap()) : 0);
}

// the partial sums of integral I of the functional M into `partials`; only_index >= 0: that entity alone (of the
// standard entities, or of the rules when use_rule), its value in partials[0].  Returns the partials written.
int64_t functional_integral(const cfx_form_s* M, const cfx_integral_dev& I, double* partials, int64_t only_index, int use_rule)
{
  const cfx_space_s* V = M->V;
  const bool single = only_index >= 0;
  if (I.type == CFX_INTERIOR_FACET) return user_stage1_facets(M, I, partials, only_index); // (registered integrands only)
  int64_t at = 0;
  const bool user = user_integrand_known(I.kernel);
  for (int part = 0; part < 2; ++part)
  {
    const bool runtime = part == 1;
    if (single && runtime != (use_rule != 0)) continue;
    if (runtime && !I.rules) continue;
    const DevN n = single ? DevN(1) : (runtime ? I.rules->nr.devn() : I.n_entities.devn());
    if (n.cap == 0) continue;
    if (user)
    {
      at += user_stage1(M, I, runtime, partials + at, 0, 0, only_index);
      continue;
    }
    FnArgs A{};
    A.x = V->mesh->x.p; A.conn = V->mesh->conn.p; A.dofmap = V->dofmap.p;
    A.n = n;
    A.qdegree = I.qdegree;
    for (int k = 0; k < 8; ++k) A.params[k] = I.params[k];
    A.coeff = I.coefficient.n > 0 ? I.coefficient.p : nullptr;
    A.partials = partials + at;
    const int64_t o = single ? only_index : 0;
    if (runtime)
    {
      // (offsets are absolute: the slices of points / weights start at offsets[e])
      A.offsets = I.rules->offsets.p + o; A.parent_map = I.rules->parent_map.p + o;
      A.points = I.rules->points.p; A.weights = I.rules->weights.p;
    }
    else
      A.entities = I.entities.p + o;
    launch_cells(V, I.kernel, A, runtime);
    at += blocks_of(n.cap);
  }
  return at;
}
} // namespace

namespace cfx
{
void functional_entity(const cfx_form_s* M, const cfx_integral_dev& I, int64_t index, int use_rule, double* out_dev)
{
  // one entity, one block, one partial: the value itself
  const int64_t written = functional_integral(M, I, out_dev, index, use_rule);
  require(written == 1, CFX_ERR_OUT_OF_RANGE, "cfx_tabulate_entity: the integral has no such entity");
}
} // namespace cfx

extern "C" {

int cfx_assemble_scalar(cfx_form_t M, double* value)
{
  CFX_API_BEGIN
  require(M && value, CFX_ERR_INVALID_ARGUMENT, "cfx_assemble_scalar: null argument");
  require(M->rank == 0, CFX_ERR_INVALID_ARGUMENT, "cfx_assemble_scalar: form is not a functional (rank 0)");
  validate_form(M);
  OutArray<double> out(value, 1, false);
  int64_t total = 0;
  for (const cfx_integral_dev& I : M->integrals) total += integral_blocks(I);
  DevArray<double> slab(total); // from the block cache, sized from the capacities
  int64_t at = 0;
  for (const cfx_integral_dev& I : M->integrals)
  {
    const int64_t written = functional_integral(M, I, slab.p + at, -1, 0);
    require(written == integral_blocks(I), CFX_ERR_RUNTIME, "cfx_assemble_scalar: partial sums out of step with the slab");
    at += written;
  }
  launch("functional_reduce", functional_reduce_kernel, dim3(1), dim3(kBlock), 0, (const double*)slab.p, total, out.dev);
  out.finish(); // a device `value`: nothing to wait for, the stream keeps running
  CFX_API_END
}

} // extern "C"
