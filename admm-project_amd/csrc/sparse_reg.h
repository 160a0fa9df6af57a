// sparse_reg.h -- argument blocks of the multi-fit robust regression on a sparse design matrix (sparse_reg.hip, DESIGN.md
// q38): K independent plain-ADMM runs of the A = D iteration (admm.m:496-743 with B = -1, c = s_k, stopcond 'standard')
// whose x-update (D'D)^-1 D'(s + z - u) is the lock-step CG of spmm_cg.h on D'D x = D'(s + z - u).  Every multi-vector
// has spmm.h's layout [chunks][len][kSpmmChunk] and every elementwise kernel spmm_cg.h's thread layout.
#pragma once
#include "spmm_cg.h"

namespace admm {

// the sums of the element pass (admm.m:621, 644-650; lad.m:148 / huberfit.m:180)
enum SrgSlot : int32_t { SR_R2 = 0, SR_AX2 = 1, SR_Z2 = 2, SR_OBJ = 3, SR_COUNT = 4 };
// the sums of the dual pass over n: ||D'(z - zprev)||^2 and ||D'u||^2 (admm.m:624, 652-654)
enum SrgDualSlot : int32_t { SD_DZ2 = 0, SD_U2 = 1, SD_COUNT = 2 };

struct SrgElemArgs {
  int64_t m;
  const double* AX;     // D x
  double* Z;
  double* U;
  double* V;            // (s + z) - u: the next right-hand side in front of D'
  double* DZ;           // z - zprev, or null: the dual residual is not evaluated
  const double* S;      // ns == 1: m values shared by all fits; ns == K: a multi-vector, one column per fit
  const double* W;      // m shared weights or null
  const double* par;    // K x 4: (a, b, epsilon, delta) of every fit
  const int32_t* kind;  // K values: 0 LAD family, 1 Huber family
  const MultiRec* rec;
  double* part;         // [chunks * kSpmmChunk][SR_COUNT][kScgMaxWg]
  int32_t K, ns, objevals;
  double rho;
};

struct SrgDualArgs {
  int64_t n;
  const double* GDZ;    // D'(z - zprev)
  const double* GU;     // D'u
  const MultiRec* rec;
  double* part;         // [chunks * kSpmmChunk][SD_COUNT][kScgMaxWg]
  int32_t K;
};

struct SrgFinArgs {
  const double* part;   // the element pass's partials, nwg per slot
  const double* dpart;  // the dual pass's partials, nwg_n per slot (dual != 0)
  const double* snorm;  // K: ||s_k||
  int64_t m;
  int32_t K, nwg, nwg_n;
  int32_t dual;         // the dual residual takes part in the stop rule (nodualerror = 0)
  MultiRec* rec;
  double *pnorm, *perr, *dnorm, *derr, *objv;  // [K][hist_ld]
  int64_t hist_ld;
  double rho, abstol, reltol;
  int32_t domaxiters, objevals, maxiters;
};

// init: V = (s + z0) - u0 only
void launch_srg_elem(const SrgElemArgs& a, bool init, hipStream_t stream);
void launch_srg_dual(const SrgDualArgs& a, hipStream_t stream);
void launch_srg_fin(const SrgFinArgs& a, hipStream_t stream);

}  // namespace admm
