#pragma once
#include "../device_tables.h"
#include "common.h"

namespace twr {
// PhaseDurations::SetVariables (phase_durations.cc:77-103) + ConvertPhaseToPolyDurations
// (nodes_variables_phase_based.cc:73-84) of one ee, spread over the lanes of a wave: loads in parallel, only the
// duration sum is serial.
TWR_DEV void phase_poly_durations_wave(const PhaseTables* PT, const char* blob, const double* __restrict__ xp, int e,
                                       double* ph, double* md, int lane, int nthreads = 64) {
  const int ns = PT->n_phases[e] - 1;
  if (lane < ns) ph[lane] = xp[PT->off_sched[e] + lane];
  __syncthreads();
  if (lane == 0) {
    double sum = 0.0;
    for (int i = 0; i < ns; ++i) sum += ph[i];
    ph[ns] = PT->t_total[e] - sum;
  }
  __syncthreads();
  const PhasePoly* mp = tbl<PhasePoly>(blob, PT->o_mpoly[e]);
  for (int q = lane; q < PT->n_mpoly[e]; q += nthreads) md[q] = ph[mp[q].phase] / mp[q].n_in_phase;
  __syncthreads();
}
}  // namespace twr
