// The launches of one evaluation, planned on the host (no HIP) from the batch's list counts and policy (eval_plan.h).
#include "eval_plan.h"

#include <algorithm>
#include <string>

namespace twr {

// The dyn / rom grids are persistent: as many workgroups as are resident at once.  Residency is LDS bound; the occupancy API
// over-reports it for the dynamic kernel (measured: 7 x 22.5 KB resident, an 8th starts a second round), so the per-CU
// counts are fixed (LaunchTuning) rather than queried.  (Running dyn and rom concurrently on two streams was measured and is
// slower than back to back.)
EvalPlan PlanEval(const EvalShape& s) {
  EvalPlan plan;
  const LaunchTuning& t = s.tuning;
  auto add = [&](Launch k, int store, int nit, int xc, int items, int grid, int block, int lds = 0) -> LaunchStep& {
    LaunchStep& p = plan.step[plan.n++];
    p.kernel = k;
    p.store = store;
    p.nit = nit;
    p.xc = xc;
    p.grid = std::min(items, grid);
    p.block = block;
    p.lds = lds;
    return p;
  };
  auto event = [&](int i) {
    if (s.events) plan.step[plan.n++].arg[0] = i;
  };
  const bool wg = s.flags & 1, wj = s.flags & 2;
  const int store = wg && wj ? kStoreGJ : wj ? kStoreJ : kStoreG;   // non-temporal stores only go with the Jacobian
  const int store_nt = !(s.stream_nt && wj) ? store : wg ? kStoreGJNT : kStoreJNT;
  const int xc = s.dyn_map_chunks == 2 ? 2 : 4;
  const int n_chunks = s.fam[0] + s.fam[1] + s.fam[2] + s.fam[3];
  auto nodes = [&]() {   // the node-based sets (terrain-*, force-*, splineacc-*, swing-*, ...): last launch of every path
    if (n_chunks > 0) {
      // persistent waves per CU for ALL families together, shared out by their chunk counts (by count, not by bytes: an iteration
      // costs about the same whatever the family -- weighting the force chunks 1.5 x ... 3 x was 4-15 % slower)
      const int res = t.node_bpc * s.n_cu;
      int gf[4], sum = 0;
      for (int f = 0; f < 4; ++f) {
        gf[f] = s.fam[f] == 0 ? 0 : std::min(s.fam[f], std::max(1, (int)((long long)res * s.fam[f] / n_chunks)));
        sum += gf[f];
      }
      LaunchStep& p = add(Launch::kChunk, store, 0, 0, sum, sum, 64);
      std::copy(gf, gf + 4, p.arg);
    } else if (s.node > 0) {
      add(s.node_families == 2 ? Launch::kNode2 : Launch::kNode, store, 0, 0, s.node, s.node, s.node_families == 2 ? 128 : 256);
    }
  };
  // Candidate scores (twr_batch_eval_scores): with score_fused the values-only launch in its scoring instantiation
  // (eval_scores_kernel: every wave reduces its rows to a partial record, the node-based sets always by the launch's own
  // node waves -- node_chunk_kernel writes g) and the fold of the partial records into the score rows; otherwise exactly
  // twr_batch_eval(TWR_EVAL_VALUES) and twr_batch_score.  Then twr_batch_best's launch if asked for.  No per-kernel events.
  if (s.flags & kEvalScores) {
    if (s.score_fused) {
      const int nx = (s.flat_max_x + 64 * kFlatGroup - 1) / (64 * kFlatGroup);
      const int n_groups = s.flat / kFlatGroup, items = n_groups + s.node;
      LaunchStep& p = add(Launch::kScores, kStoreG, 0, nx <= 3 ? 3 : nx <= 5 ? 5 : 8, items, items, 64 * kFlatGroup, flat_lds_bytes(s.flat_max_x));
      p.arg[0] = n_groups;
      p.arg[1] = s.node_families;
      p.arg[2] = flat_x_bytes(s.flat_max_x);
      const int fold = (kFoldThreads * s.node + 255) / 256;
      add(Launch::kFold, kStoreG, 0, 0, fold, fold, 256).arg[0] = s.node;
    } else {
      EvalShape v = s;
      v.flags = 1;   // TWR_EVAL_VALUES
      v.events = false;
      plan = PlanEval(v);
      add(Launch::kScoreG, kStoreG, 0, 0, s.node, s.node, 256).arg[0] = s.node;
    }
    if (s.flags & kEvalBest) {   // (launch_best's grid: four candidates per thread, at most 256 workgroups)
      const int blocks = std::max(1, std::min((s.node + 1023) / 1024, 256));
      add(Launch::kBest, kStoreG, 0, 0, blocks, blocks, 256).arg[0] = s.node;
    }
    return plan;
  }
  // Values only (no Jacobian), every problem with fixed timings and at most kFlatXCap variables: "dynamic" and "rangeofmotion-*"
  // with one lane per time node (flat items), the node-based sets -- one launch (eval_values_kernel); with per-kernel events three.
  if (wg && !wj && s.flat > 0 && s.pdyn == 0 && s.prom == 0 && s.ploc == 0) {
    const int nf = !s.events && n_chunks == 0 ? s.node_families : 0;   // (large batches: the chunk kernel takes the node sets;
                                                                        // with per-kernel events they are a launch of their own)
    const int nx = (s.flat_max_x + 64 * kFlatGroup - 1) / (64 * kFlatGroup);
    static_assert(kFlatXCap <= 8 * 64 * kFlatGroup, "largest instantiation of the values-only kernel");
    const int n_groups = s.flat / kFlatGroup, items = n_groups + (nf > 0 ? s.node : 0);
    event(0);
    LaunchStep& p = add(Launch::kValues, kStoreG, 0, nx <= 3 ? 3 : nx <= 5 ? 5 : 8, items, items, 64 * kFlatGroup, flat_lds_bytes(s.flat_max_x));
    p.arg[0] = n_groups;
    p.arg[1] = nf;
    p.arg[2] = flat_x_bytes(s.flat_max_x);
    event(1);   // (the two flat families are one launch: the second interval is empty)
    event(2);
    if (nf == 0) nodes();
    event(3);
    return plan;
  }
  const int cap = t.rom_bpc * s.n_cu;
  // The fused launch (the dyn, rom and node roles as blocks of one launch) is used while the rom role needs at most TWENTY
  // rounds of its residency (rom_bpc workgroups per CU x n_cu).  Round-3 re-tune on one box, ragged sweep, fused vs three
  // launches: 320 / 400 / 512 candidates 75 / 98 / 126 vs 83 / 104 / 128 us per step, 768 / 1024: 187 / 250 vs 183 / 235;
  // round 4: 512 candidates 115 vs 124, 768 / 1024 equal.  The 512 candidates of a two-GPU shard of the C5 sweep are ~8500
  // rom slices (the enumeration is ragged: 16.6 slices per candidate), 8.3 rounds on the 256 CUs of an MI355X.  With
  // non-temporal stores (sweep-like batches) the fused launch stays ahead for longer -- 768 / 896 / 1024 candidates of the
  // C5 sweep (12.7 / 14.9 / 17 thousand rom slices): 160-165 / 179 / 210 us as three launches, 148 / 166 / 202 us fused --
  // twenty rounds there (the enumeration ends at 1040 candidates; nothing larger was measured).  Round 5, with the roles
  // always co-resident: batches that share one structure, plain stores, 640 / 1024 / 2048 problems 129.5 / 193.5 / 365 us as
  // three launches, 120 / 188 / 376 us fused -- twenty rounds for both store policies.  The thresholds are in units of the
  // device's residency, not constants of one chip.
  const int fused_max = t.fused_max_rom > 0 ? t.fused_max_rom : 20 * cap;
  if (!s.events && s.pdyn == 0 && s.prom == 0 && s.rom > 0 && s.dyn > 0 && s.rom <= fused_max) {
    const int half_dyn = (s.dyn + 1) / 2;
    int g_rom = std::min(s.rom, cap), g_dyn = std::min(half_dyn, cap);
    // When the two persistent roles do not fit the CUs together, the blocks of the later role only start as the earlier
    // ones retire, i.e. the roles run one after the other.  For up to 2560 rom slices (160 quadruped candidates of
    // K = 200) it pays to give each role half of the residency instead, so that the latency-bound dyn waves and the
    // store-bound rom waves overlap from the start (64 / 128 / 160 candidates: 18.7 / 30.1 / 35.2 -> 17.5 / 27.8 /
    // 31.6 us per step; from 200 candidates on the extra rounds cost more than the overlap gains).
    // (round 3: five eighths for rom up to 3200 slices -- 128 / 160 / 200 candidates 27.5 / 33.5 / 40.5 us against 27.7 / 33.9 /
    // 44.0 us with the round-2 rule "half each up to 2560"; from 256 candidates on unsplit was as good or better THEN.)
    // Round 5, re-measured with the round-4 kernels (split tables, nt stores; one box, ragged sweep, us per step unsplit ->
    // split): 256 candidates 53.8 -> 47.2 (five eighths; 48.6 at four), 320: 69.3 -> 62.5 (four), 384: 81.7 -> 74.5, 512:
    // 100.9 -> 92.6, 768: 155.8 -> 145.9, 1024: 206.0 -> 194.1; six eighths loses everywhere.  The two roles are ALWAYS
    // co-resident now: the latency-bound dyn waves fill the holes of the store-bound rom stream.
    const int split = t.fused_split > 0 ? t.fused_split : (8 * s.rom <= 34 * cap ? 5 : 4);   // (4352 slices on 256 CUs)
    if (split < 8 && g_rom + g_dyn > cap) {   // split = eighths of the residency given to rom (8 = never split)
      g_rom = std::min(g_rom, cap * split / 8);
      g_dyn = std::min(g_dyn, cap - cap * split / 8);
    }
    if (t.fused_grom > 0) g_rom = std::min(t.fused_grom, s.rom);
    if (t.fused_gdyn > 0) g_dyn = std::min(t.fused_gdyn, half_dyn);
    if (g_dyn >= 8) g_dyn &= ~7;   // (the XCD-aware slice mapping of the dyn role, eval_fused_kernel)
    const int need = (s.rom_max_vals + 1 + 2 + 127) / 128;   // copy-out length of the rom role (as for rom_kernel below)
    const int grid = g_rom + g_dyn + 2 * s.node;
    LaunchStep& p = add(Launch::kFused, store_nt, need <= 34 ? 34 : kRomNitMax, xc, grid, grid, 128);
    p.arg[0] = g_rom;
    p.arg[1] = g_dyn;
    return plan;
  }
  event(0);
  if (s.dyn > 0) {
    LaunchStep& p = add(Launch::kDyn, store_nt, 0, xc, s.dyn, t.dyn_bpc * s.n_cu, 64);
    // A uniform list (BatchPlan::dyn_uniform) goes to dyn_uniform_kernel, whose waves own one slice kind each and load its
    // records once per launch, when the grid divides into kinds without idling the residency (DynUniformCols).
    const int cols = DynUniformCols(s.dyn_uniform.s, s.dyn_uniform.n_problems, t.dyn_bpc * s.n_cu);
    if (cols > 0 && s.dyn == s.dyn_uniform.s * s.dyn_uniform.n_problems) {
      p.uni = s.dyn_uniform;
      p.uni.cols = cols;
      p.grid = 8 * p.uni.s * cols;
    }
  }
  // optimised-timings problems: the pre-pass (segment lookup -> records), then the persistent kernels; their LDS per
  // workgroup is the image of one pass, and their residency follows from it
  if (s.ploc > 0) add(Launch::kLocate, store, 0, 0, s.ploc, s.ploc, kLocateThreads);
  auto phase_bpc = [&](int lds, int most, int knob) { return knob > 0 ? knob : std::max(1, std::min(most, 160 * 1024 / lds)); };
  if (s.pdyn > 0) {   // (at most one wave per SIMD: the kernel uses the AGPR half of the register file as well)
    const int lds = 8 * ((s.pdyn_img_cap + 1) & ~1);
    add(Launch::kDynPhase, store, s.pdyn_img_cap <= 40 * 128 ? 40 : 0, 0, s.pdyn, phase_bpc(lds, 4, t.pdyn_bpc) * s.n_cu, 64, lds);
  }
  event(1);
  if (s.prom > 0) {
    const int lds = 8 * ((s.prom_img_cap + 1) & ~1), img = s.prom_img_cap;
    const int nit = img <= 24 * 128 ? 24 : img <= 32 * 128 ? 32 : img <= 40 * 128 ? 40 : 0;
    add(Launch::kRomPhase, store, nit, 0, s.prom, phase_bpc(lds, 8, t.prom_bpc) * s.n_cu, 64, lds);
  }
  if (s.rom > 0) {
    // NIT = store instructions of rom_kernel's copy-out: the smallest instantiation that covers the largest slice of the
    // batch (+ parity shift, rounded up to whole store instructions).  The stores past the end of a slice are re-stores of its
    // last pair -- no HBM traffic, but requests all the same: C3's balanced 50-node slices need 34, and 34 instead of 38 is
    // worth 4 % of the kernel (A/B on one box: 0.925 -> 0.883 ms together with the balanced slices; five 40-node slices with
    // 27 stores each: 0.965 ms -- large slices win).
    const int need = (s.rom_max_vals + 1 + 2 + 127) / 128;
    add(Launch::kRom, store_nt, need <= 26 ? 26 : need <= 30 ? 30 : need <= 34 ? 34 : kRomNitMax, 0, s.rom, cap, 64);
  }
  event(2);
  nodes();
  event(3);
  return plan;
}

const char* StoreName(int store) {
  switch (store) {
    case kStoreG: return "G";
    case kStoreJ: return "J";
    case kStoreGJ: return "GJ";
    case kStoreJNT: return "JNT";
    case kStoreGJNT: return "GJNT";
  }
  return "?";
}

const char* KernelName(const LaunchStep& p) {
  switch (p.kernel) {
    case Launch::kEvent: return "";
    case Launch::kDyn: return p.uni.s > 0 ? "dyn_uniform_kernel" : "dyn_kernel";
    case Launch::kRom: return "rom_kernel";
    case Launch::kFused: return "eval_fused_kernel";
    case Launch::kLocate: return "phase_locate_kernel";
    case Launch::kDynPhase: return "dyn_phase_kernel";
    case Launch::kRomPhase: return "rom_phase_kernel";
    case Launch::kNode: return "node_kernel";
    case Launch::kNode2: return "node_kernel2";
    case Launch::kChunk: return "node_chunk_kernel";
    case Launch::kValues: return "eval_values_kernel";
    case Launch::kScores: return "eval_scores_kernel";
    case Launch::kFold: return "score_fold_kernel";
    case Launch::kScoreG: return "score_kernel";
    case Launch::kBest: return "best_kernel";
  }
  return "?";
}

std::string InstantiationName(const LaunchStep& p) {
  const std::string k = KernelName(p), st = StoreName(p.store);
  switch (p.kernel) {
    case Launch::kDyn: return k + "<" + st + ",xc" + std::to_string(p.xc) + ">";
    case Launch::kRom:
    case Launch::kDynPhase:
    case Launch::kRomPhase: return k + "<" + std::to_string(p.nit) + "," + st + ">";
    case Launch::kFused: return k + "<" + std::to_string(p.nit) + ",xc" + std::to_string(p.xc) + "," + st + ">";
    case Launch::kChunk: return k + "<" + st + ">";
    case Launch::kValues:
    case Launch::kScores: return k + "<" + std::to_string(p.xc) + ">";
    default: return k;
  }
}

}  // namespace twr
