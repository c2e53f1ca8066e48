// Batch planning on the host (no HIP): everything twr_batch_create uploads besides the structures' tables -- the offsets
// of every problem, every work list in launch order and the batch's policy decisions (batch_plan.h).
#include "batch_plan.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace twr {

LayoutShare ShareLayoutTables(const std::vector<const Structure*>& structs) {
  struct Seen {
    const char* bytes;
    uint32_t n;
    LayoutShare::Ref ref;
  };
  auto hash = [](const char* p, size_t n) {   // FNV-1a over 8-byte words (a bucket key only: equality is decided by memcmp)
    uint64_t h = 1469598103934665603ull;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      std::memcpy(&w, p + i, 8);
      h = (h ^ w) * 1099511628211ull;
      h ^= h >> 29;
    }
    for (; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    return h;
  };
  LayoutShare out;
  out.of.resize(structs.size());
  std::unordered_map<uint64_t, std::vector<Seen>> by_hash;
  for (size_t i = 0; i < structs.size(); ++i) {
    const Structure& S = *structs[i];
    for (const Structure::TableRef& tr : S.dyn_layout_tables) {
      if ((size_t)tr.off + tr.bytes > S.blob.size()) throw std::runtime_error("layout table outside its blob");
      const char* src = S.blob.data() + tr.off;
      std::vector<Seen>& bucket = by_hash[hash(src, tr.bytes) ^ tr.bytes];
      LayoutShare::Ref ref{(int)i, tr.off};
      bool found = false;
      for (const Seen& sn : bucket)
        if (sn.n == tr.bytes && std::memcmp(sn.bytes, src, tr.bytes) == 0) {
          ref = sn.ref;
          found = true;
          break;
        }
      if (!found) {
        bucket.push_back({src, tr.bytes, ref});
        out.bytes_distinct += tr.bytes;
      }
      out.bytes_built += tr.bytes;
      out.of[i].push_back(ref);
    }
  }
  return out;
}

std::vector<size_t> BlobOffsets(const std::vector<const Structure*>& structs) {
  std::vector<size_t> off(structs.size() + 1, 0);
  for (size_t i = 0; i < structs.size(); ++i) off[i + 1] = off[i] + (structs[i]->blob.size() + 255) / 256 * 256;
  return off;
}

namespace {
// XCD-aware order.  Workgroups are dealt round-robin over the 8 XCDs and the persistent grids are multiples of 8, so list
// position j runs on XCD j % 8 (eval_fused_kernel's slice mapping relies on it, kernels/fused.h).  Interleaving the problems in
// groups of 8 puts all items of one problem on ONE XCD (same L2): its x is fetched from HBM once per kernel instead of once
// per XCD.  (Speed only; ragged item counts merely loosen the alignment.)  first: first item of every problem (+ end).
template <class W>
void Interleave(std::vector<W>& items, const std::vector<int>& first) {
  const std::vector<W> src = items;
  const int n = (int)first.size() - 1;
  size_t out = 0;
  for (int p0 = 0; p0 < n; p0 += 8) {
    const int np = std::min(8, n - p0);
    for (int s = 0;; ++s) {
      bool any = false;
      for (int k = 0; k < np; ++k)
        if (first[p0 + k] + s < first[p0 + k + 1]) {
          items[out++] = src[first[p0 + k] + s];
          any = true;
        }
      if (!any) break;
    }
  }
}
}  // namespace

void BatchPlan::PlaceRecords(uint64_t base) {
  for (auto& lw : lists.ploc) {
    if (lw.recs) lw.recs += base - 1;
    if (lw.dyn_loc) lw.dyn_loc += base - 1;
  }
  for (auto& rw : lists.prom) rw.recs += base;
  for (auto& pw : lists.pdyn) pw.loc += base;
}

namespace {
// What the builders of a batch's plan share: PlanBatch's arguments and what the first builders work out for the later ones.
// Every builder below fills the part of the BatchPlan its name says and nothing else.
struct BatchInputs {
  const std::vector<const Structure*>& structs;
  const std::vector<int32_t>& struct_of_problem;
  const std::vector<uint64_t>& blob_at;
  std::vector<std::unordered_map<uint32_t, uint64_t>> layout_at;   // [structure][blob offset of the table] -> device address
  std::vector<uint64_t> model_hdr;                                 // [structure] the DevStruct header its dyn slices read
  std::vector<int> flat_group_p;                                   // the problem of every group of four flat items
  bool flat_ok = true;                                             // every problem can take the values-only path
  int n_problems() const { return (int)struct_of_problem.size(); }
  const Structure& of(int p) const { return *structs[struct_of_problem[p]]; }
  const DevStruct* header(int p) const { return reinterpret_cast<const DevStruct*>(of(p).blob.data()); }
};

// Layout tables of dyn_kernel (device_tables.h) are stored once per distinct CONTENT: a structure whose table is
// byte-identical to one of an earlier structure of the batch reads that one (its own copy stays in the arena, unread).
// Candidates of a sweep that differ in the total time only share all of them, and an evaluation then reads 24 B per
// time node + 16 B per polynomial of such a candidate instead of ~35 KB.  The model constants (DevStruct header) are
// taken from the first structure of the batch that has the same ones.
void ShareLayouts(BatchInputs& in, BatchPlan& b) {
  const auto& structs = in.structs;
  const int n_structs = (int)structs.size();
  in.layout_at = std::vector<std::unordered_map<uint32_t, uint64_t>>(n_structs);
  in.model_hdr = std::vector<uint64_t>(n_structs);
  const LayoutShare share = ShareLayoutTables(structs);
  b.dyn_layout_bytes = share.bytes_built;
  b.dyn_layout_distinct_bytes = share.bytes_distinct;
  for (int i = 0; i < n_structs; ++i) {
    const auto& tabs = structs[i]->dyn_layout_tables;
    for (size_t t = 0; t < tabs.size(); ++t) in.layout_at[i][tabs[t].off] = in.blob_at[share.of[i][t].owner] + share.of[i][t].off;
    const DevStruct* H = reinterpret_cast<const DevStruct*>(structs[i]->blob.data());
    in.model_hdr[i] = in.blob_at[i];
    for (int q = 0; q < i; ++q) {
      const DevStruct* Q = reinterpret_cast<const DevStruct*>(structs[q]->blob.data());
      if (in.model_hdr[q] == in.blob_at[q] && Q->mass == H->mass && Q->gravity == H->gravity && std::memcmp(Q->Ib, H->Ib, sizeof(H->Ib)) == 0) {
        in.model_hdr[i] = in.model_hdr[q];
        break;
      }
    }
    if (structs[i]->dyn_staged_max > 128) b.dyn_map_chunks = 4;
  }
}

// Every problem's offsets, what twr_batch_sample needs of it, and its entry of the node list
void PlaceProblems(const BatchInputs& in, BatchPlan& b) {
  const int n_structs = (int)in.structs.size(), n_problems = in.n_problems();
  b.x_off.assign(n_problems + 1, 0);
  b.g_off.assign(n_problems + 1, 0);
  b.j_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = in.struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    const Structure& S = in.of(p);
    const uint64_t blob = in.blob_at[si];
    const SampleTables* st = reinterpret_cast<const SampleTables*>(S.blob.data() + in.header(p)->o_sample);
    b.blob_of_problem.push_back(blob);
    b.t_total.push_back(st->t_total);
    b.sample_ok.push_back(st->n_base >= 0);
    b.x_off[p + 1] = b.x_off[p] + S.n_vars;
    b.g_off[p + 1] = b.g_off[p] + S.n_rows;
    b.j_off[p + 1] = b.j_off[p] + S.nnz;
    NodeWork nw;
    nw.blob = blob;
    nw.x_off = b.x_off[p];
    nw.g_off = b.g_off[p];
    nw.j_off = b.j_off[p];
    b.lists.node.push_back(nw);
  }
  // one entry past the end carries the totals: a kernel reads a problem's row count as work[p + 1].g_off - work[p].g_off
  // from the work list alone (score_kernel requests g before the structure's header has arrived)
  b.lists.node.push_back(NodeWork{0, b.x_off[n_problems], b.g_off[n_problems], b.j_off[n_problems]});
}

// The dyn and rom lists: the slices of the problems with fixed timings (a structure with optimised timings has none; a
// family that is switched off -- twr_params.constraint_sets -- simply has no work items), in XCD order
void AddSliceItems(const BatchInputs& in, BatchPlan& b) {
  BatchPlan::Lists& L = b.lists;
  std::vector<int> dyn_first, rom_first;   // first work item of every problem (+ end)
  for (int p = 0; p < in.n_problems(); ++p) {
    const int si = in.struct_of_problem[p];
    const Structure& S = in.of(p);
    const uint64_t blob = b.blob_of_problem[p];
    dyn_first.push_back((int)L.dyn.size());
    rom_first.push_back((int)L.rom.size());
    const SetInfo* dsp = S.FindSet("dynamic");
    const SetInfo ds = dsp ? *dsp : SetInfo();
    for (const auto& sl : S.dyn_slices) {
      DynWork w;
      std::memset(&w, 0, sizeof(w));
      const auto& lay = in.layout_at[si];
      w.nodes_t = blob + S.off_dyn_nodes_t + sizeof(DynNodeT) * (size_t)sl.k0;
      w.nodes_l = lay.at(S.off_dyn_nodes_l) + sizeof(DynNodeL) * (size_t)sl.k0;
      w.sel = lay.at(S.off_dyn_sel) + sizeof(DynSel) * (size_t)sl.k0 * 4;
      w.tile = lay.at(S.off_dyn_tile);   // (records are addressed through DynSel::tile)
      w.poly_t = blob + S.off_dyn_poly_t + sizeof(DynPolyT) * (size_t)sl.poly0;
      w.poly_l = lay.at(S.off_dyn_poly_l) + sizeof(DynPolyL) * (size_t)sl.poly0;
      w.map = lay.at(b.dyn_map_chunks == 2 ? sl.map2 : sl.map);
      w.hdr = in.model_hdr[si];
      w.x_off = b.x_off[p];
      w.g_off = b.g_off[p] + ds.offset + 6 * sl.k0;
      w.j_off = b.j_off[p] + S.row_ptr[ds.offset + 6 * sl.k0];
      w.cnt = sl.cnt;
      w.nvals = sl.nvals;
      L.dyn.push_back(w);
    }
    for (int e = 0; e < (int)S.rom_slices.size(); ++e) {
      if (S.rom_slices[e].empty()) continue;
      const SetInfo& rs = *S.FindSet("rangeofmotion-" + std::to_string(e));
      for (const auto& sl : S.rom_slices[e]) {
        RomWork w;
        std::memset(&w, 0, sizeof(w));
        w.nodes = blob + S.off_rom_nodes + sizeof(RomNode) * (size_t)sl.k0;
        w.segs = blob + sl.segs;
        w.x_off = b.x_off[p];
        w.g_off = b.g_off[p] + rs.offset + 3 * sl.k0;
        w.j_off = b.j_off[p] + S.row_ptr[rs.offset + 3 * sl.k0];
        w.off_lin = S.off_base_lin;
        w.off_ang = S.off_base_ang;
        w.cnt = sl.cnt;
        w.nvals = sl.nvals;
        w.ee = e;
        b.rom_max_vals = std::max(b.rom_max_vals, w.nvals);
        L.rom.push_back(w);
      }
    }
  }
  dyn_first.push_back((int)L.dyn.size());
  rom_first.push_back((int)L.rom.size());
  Interleave(L.dyn, dyn_first);
  Interleave(L.rom, rom_first);
}

// The lists of the problems with optimised timings (PDynWork / LocWork / RomPhaseWork instead of DynWork / RomWork), the
// scratch their x-dependent records take (records_bytes) and the LDS images of the two phase kernels
void AddPhaseItems(const BatchInputs& in, BatchPlan& b) {
  BatchPlan::Lists& L = b.lists;
  std::vector<int> pdyn_first;   // first PDynWork of every problem that has some (+ end)
  for (int p = 0; p < in.n_problems(); ++p) {
    const Structure& S = in.of(p);
    if (!S.timings) continue;
    const DevStruct* H = in.header(p);
    const uint64_t blob = b.blob_of_problem[p];
    const SetInfo* dsp = S.FindSet("dynamic");
    const int Kd = (int)S.grid_dyn.size();
    const size_t loc_off = b.records_bytes;   // DynLoc[4 * Kd] of this problem, then its RomRec arrays
    const PhaseTables& pt = S.phase_tables;
    if (dsp) {
      // dyn_phase_kernel: a pass = the time nodes whose expanded rows fit the LDS image (four at sixteen lanes each,
      // fewer when a node has more than 5120 values: the image then takes the whole 160 KB of a CU)
      b.records_bytes += sizeof(DynLoc) * 4 * (size_t)Kd;
      const int nv = pt.node_vals;
      const int run = std::max(1, std::min(4, (160 * 128) / nv));
      b.pdyn_img_cap = std::max(b.pdyn_img_cap, run * nv);
      pdyn_first.push_back((int)L.pdyn.size());
      for (int k0 = 0; k0 < Kd; k0 += run) {
        PDynWork pw;
        std::memset(&pw, 0, sizeof(pw));
        pw.hdr = blob;
        pw.loc = loc_off + sizeof(DynLoc) * (size_t)k0;
        pw.loc_stride = (int32_t)(sizeof(DynLoc) * (size_t)Kd);
        pw.shared = blob + pt.o_dyn_shared + sizeof(DynShared) * (size_t)k0;
        pw.mput = blob + pt.o_mput;
        pw.fput = blob + pt.o_fput;
        pw.ee = blob + H->o_phase + offsetof(PhaseTables, ee);
        pw.x_off = b.x_off[p];
        pw.g_off = b.g_off[p] + dsp->offset + 6 * k0;
        pw.j_off = b.j_off[p] + dsp->nnz_offset + (int64_t)k0 * nv;
        pw.cnt = std::min(run, Kd - k0);
        pw.node_vals = nv;
        pw.off_lin = S.off_base_lin;
        pw.off_ang = S.off_base_ang;
        pw.n_ee = S.n_ee;
        pw.n_mput = pt.n_mput;
        pw.n_fput = pt.n_fput;
        for (int q = 0; q < 5; ++q) pw.row_off[q] = pt.dyn_row_off[q];
        L.pdyn.push_back(pw);
      }
    }
    for (int e = 0; e < S.n_ee; ++e) {
      const SetInfo* rs = S.FindSet("rangeofmotion-" + std::to_string(e));
      if (!rs && !dsp) continue;
      LocWork lw;
      std::memset(&lw, 0, sizeof(lw));
      lw.blob = blob;
      lw.recs = rs ? b.records_bytes + 1 : 0;   // (+1: see BatchPlan::records_bytes)
      lw.dyn_loc = dsp ? loc_off + sizeof(DynLoc) * (size_t)Kd * (size_t)e + 1 : 0;
      lw.x_off = b.x_off[p];
      lw.ee = e;
      L.ploc.push_back(lw);
      if (!rs) continue;
      const int K = (int)S.grid_rom.size(), nv = pt.rom_node_vals[e];
      const int run_max = std::max(1, std::min(16, (160 * 128) / nv));   // time nodes per pass (four lanes each)
      const int n_pass = (K + run_max - 1) / run_max;
      const int run = (K + n_pass - 1) / n_pass;                  // balanced: no short tail pass (it pays the full copy-out)
      b.prom_img_cap = std::max(b.prom_img_cap, run * nv);
      for (int k0 = 0; k0 < K; k0 += run) {
        RomPhaseWork rw;
        rw.recs = b.records_bytes + sizeof(RomRec) * (size_t)k0;
        rw.x_off = b.x_off[p];
        rw.g_off = b.g_off[p] + rs->offset + 3 * k0;
        rw.j_off = b.j_off[p] + rs->nnz_offset + (int64_t)k0 * nv;
        rw.off_lin = S.off_base_lin;
        rw.off_ang = S.off_base_ang;
        rw.cnt = std::min(run, K - k0);
        rw.msize = pt.msize[e];
        rw.ns = S.schedule.n_phases[e] - 1;
        rw.node_vals = nv;
        L.prom.push_back(rw);
      }
      b.records_bytes += sizeof(RomRec) * (size_t)K;
    }
  }
  pdyn_first.push_back((int)L.pdyn.size());
  Interleave(L.pdyn, pdyn_first);
}

// The values-only work items of one problem's grid (device_tables.h FlatWork): 64 time nodes of the dynamic /
// range-of-motion grid each
void AddFlatItems(const BatchInputs& in, BatchPlan& b, int p, uint32_t off_nodes, const std::vector<Structure::FlatItem>& list, bool dynamic) {
  const Structure& S = in.of(p);
  const DevStruct* H = in.header(p);
  const uint64_t blob = b.blob_of_problem[p];
  for (const auto& it : list) {
    FlatWork fw;
    std::memset(&fw, 0, sizeof(fw));
    fw.nodes = blob + off_nodes + sizeof(FlatNode) * (size_t)it.k0;
    fw.polys = blob + S.off_flat_polys;
    fw.x_off = b.x_off[p];
    fw.g_off = b.g_off[p];
    fw.k0 = it.k0;
    fw.cnt = it.cnt;
    fw.start[0] = it.start[0];
    fw.start[1] = it.start[1];
    fw.count = it.count;
    fw.n_x = S.n_vars;
    fw.n_ee = S.n_ee;
    fw.off_lin = S.off_base_lin;
    fw.off_ang = S.off_base_ang;
    for (int e = 0; e < kMaxEE; ++e) fw.row_rom[e] = S.flat_row_rom[e];
    fw.dynamic = dynamic ? 1 : 0;
    fw.gather = it.gather ? 1 : 0;
    if (dynamic) {
      fw.row_dyn = S.flat_row_dyn;
      fw.with_rom = S.flat_with_rom ? 1 : 0;
      fw.mass = H->mass;
      fw.gravity = H->gravity;
      for (int i = 0; i < 6; ++i) fw.Ib[i] = H->Ib[i];
    }
    b.lists.flat.push_back(fw);
  }
}

// The flat list in problem order, in whole groups of four per problem, and whether every problem can take the values-only
// path at all (flat_ok: none has optimised timings, and none has a dynamic / range-of-motion set without flat tables)
void AddFlatGroups(BatchInputs& in, BatchPlan& b) {
  BatchPlan::Lists& L = b.lists;
  for (int p = 0; p < in.n_problems(); ++p) {
    const Structure& S = in.of(p);
    if (S.timings) in.flat_ok = false;
    if (S.off_flat_polys) {
      b.flat_max_x = std::max(b.flat_max_x, S.n_vars);
      AddFlatItems(in, b, p, S.off_flat_dyn, S.flat_items_dyn, true);
      AddFlatItems(in, b, p, S.off_flat_rom, S.flat_items_rom, false);
      while (L.flat.size() % 4 != 0) {   // whole groups: empty items that still carry the problem's x (the group copies it
        FlatWork fw;                     // to LDS with all its threads)
        std::memset(&fw, 0, sizeof(fw));
        fw.x_off = b.x_off[p];
        fw.n_x = S.n_vars;
        L.flat.push_back(fw);
      }
      in.flat_group_p.resize(L.flat.size() / 4, p);
    } else if (S.FindSet("rangeofmotion-0") || S.FindSet("dynamic")) {
      in.flat_ok = false;
    }
  }
}

// The policy scalars: dyn_uniform, stream_nt, node_families
void DecidePolicy(const BatchInputs& in, BatchPlan& b, int64_t cache_bytes) {
  const auto& struct_of_problem = in.struct_of_problem;
  const int n_problems = in.n_problems();
  // Uniform dyn list: one structure with fixed timings for every problem -- in the flagship batch and in its real use, many
  // x for one NLP -- so problem p's slice of a kind is problem 0's with x, g and jac moved on by p strides.  (By structure
  // INDEX: two equal structures are two tables in the arena, and a batch of them takes the general kernel.)  The interleaved
  // order puts problem 0's slices min(8, n) positions apart.
  bool one = n_problems > 0;
  for (int si : struct_of_problem) one = one && si == struct_of_problem[0];
  if (one) {
    const Structure& S = in.of(0);
    const int s = (int)S.dyn_slices.size();
    if (!S.timings && s > 0 && b.lists.dyn.size() == (size_t)s * (size_t)n_problems)
      b.dyn_uniform = DynUniform{s, 0, std::min(8, n_problems), n_problems, S.n_vars, S.n_rows, S.nnz, 0};
  }
  // Store policy of the copy-out (kernels/copy_out.h copy_out_fixed): non-temporal when the batch is SWEEP-LIKE -- fewer than four
  // problems per structure on average, so every evaluation re-reads tables (and x) that only that problem uses -- AND one
  // evaluation writes more than the device's memory-side cache holds (256 MB on an MI355X; by architecture name, batch_plan.h), so that plain stores would flush those
  // tables out of it between two evaluations.  Measured (one box, no per-kernel events): the C5 sweep at 512 /
  // 1024 candidates 116-118 / 223-224 -> 99 / 209-211 us per step; at 256 candidates (220 MB of output, absorbed by the
  // Infinity Cache as it is) 52 -> 55 us, and 8192 problems of ONE structure lose 15 % in rom_kernel -- hence the two conditions.
  std::vector<char> used(in.structs.size(), 0);
  int n_used = 0;
  for (int si : struct_of_problem)
    if (!used[si]) {
      used[si] = 1;
      ++n_used;
    }
  b.stream_nt = StreamNonTemporal(n_used, n_problems, 8 * (b.g_off[n_problems] + b.j_off[n_problems]), cache_bytes);
  b.node_families = 2;
  for (const Structure* S : in.structs)
    if (S->params.constraint_sets & ~(TWR_SET_TERRAIN | TWR_SET_DYNAMIC | TWR_SET_ROM | TWR_SET_FORCE)) b.node_families = 4;
}

// The flat groups in launch order, and the scoring lists that go with it (no flat list at all unless flat_ok)
void OrderFlatGroups(const BatchInputs& in, BatchPlan& b) {
  BatchPlan::Lists& L = b.lists;
  const std::vector<int>& flat_group_p = in.flat_group_p;
  const int n_problems = in.n_problems();
  if (!in.flat_ok) {
    L.flat.clear();
    return;
  }
  // One problem, one XCD: workgroup r of the launch runs on XCD r modulo 8 and takes group r.  The groups of problem p go to
  // workgroups = p modulo 8: its x comes from HBM once and from that XCD's L2 for its other groups.
  std::vector<size_t> queue[8];   // queue c: the groups that go to the list positions = c modulo 8
  for (size_t i = 0; i < flat_group_p.size(); ++i) queue[flat_group_p[i] % 8].push_back(i);
  std::vector<FlatWork> out;
  out.reserve(L.flat.size());
  std::vector<size_t> order;      // the groups in list order
  order.reserve(flat_group_p.size());
  auto emit = [&](size_t group) {
    out.insert(out.end(), L.flat.begin() + 4 * group, L.flat.begin() + 4 * group + 4);
    order.push_back(group);
  };
  size_t depth = 0, k = 0;
  for (const auto& q : queue) depth = std::max(depth, q.size());
  for (; k < depth; ++k) {   // whole rounds of eight; a round in which a queue has run dry ends the interleaving
    bool whole = true;
    for (const auto& q : queue) whole = whole && k < q.size();
    if (!whole) break;
    for (const auto& q : queue) emit(q[k]);
  }
  for (const auto& q : queue)
    for (size_t i = k; i < q.size(); ++i) emit(q[i]);
  // candidate scoring without g: where every group went, then per problem its partial records in a fixed order (its groups
  // in the order the structure lists its items, so the fold's sums do not depend on where the problem sits in the batch)
  std::vector<int32_t> pos(flat_group_p.size());
  for (size_t i = 0; i < order.size(); ++i) pos[order[i]] = (int32_t)i;
  const int32_t n_groups = (int32_t)flat_group_p.size();
  L.score_blob.resize(order.size());
  for (size_t i = 0; i < order.size(); ++i) L.score_blob[i] = b.blob_of_problem[flat_group_p[order[i]]];
  L.score_first.assign(1, 0);
  size_t i = 0;
  for (int p = 0; p < n_problems; ++p) {
    for (; i < flat_group_p.size() && flat_group_p[i] == p; ++i)
      for (int w = 0; w < kFlatGroup; ++w)
        if (L.flat[kFlatGroup * i + w].cnt > 0) L.score_slot.push_back(kFlatGroup * pos[i] + w);   // (L.flat: still in list order)
    for (int w = 0; w < b.node_families; ++w) L.score_slot.push_back(kFlatGroup * (n_groups + p) + w);
    L.score_first.push_back((int32_t)L.score_slot.size());
  }
  b.score_fused = true;
  b.score_slab = (int64_t)kFlatGroup * (n_groups + n_problems);
  L.flat.swap(out);
}

// Large batches whose node-based sets are terrain / force / splineacc / swing only: per-family chunk lists for the
// persistent node_chunk_kernel (baseMotion and totalduration rows, and small batches -- where the fused launch or the
// one-workgroup-per-problem kernel is as good -- stay with node_kernel).
// (hot-path batches -- terrain and force rows only -- are faster on node_kernel2: 0.041 vs 0.047 ms per 8192 C3 problems)
// (from eight problems per CU on -- 2048 on the 256 CUs of an MI355X, where the cut-over was measured: below that the
// one-workgroup-per-problem kernel has enough waves in flight and no persistent loop to fill)
void AddFamilyChunks(const BatchInputs& in, BatchPlan& b, int n_cu, int force_chunk) {
  const int n_problems = in.n_problems();
  bool eligible = n_problems >= 8 * n_cu && b.node_families == 4;
  for (const Structure* S : in.structs)
    if (S->params.constraint_sets & (TWR_SET_BASE_ROM | TWR_SET_TOTAL_TIME)) eligible = false;
  for (int p = 0; p < n_problems && eligible; ++p) {
    const DevStruct* H = in.header(p);
    auto add = [&](int f, int count, uint32_t table_off, size_t rec_bytes, int row0, int rows_per, int nnz0, int vals_per) {
      const int chunk = f == 1 ? force_chunk : 64;
      for (int i0 = 0; i0 < count; i0 += chunk) {
        FamWork w;
        std::memset(&w, 0, sizeof(w));
        w.blob = b.blob_of_problem[p];
        w.table = w.blob + table_off + (f == 2 ? 0 : rec_bytes * (size_t)i0);
        w.x_off = b.x_off[p];
        w.g_off = b.g_off[p] + row0 + (int64_t)rows_per * i0;
        w.j_off = b.j_off[p] + nnz0 + (int64_t)vals_per * i0;
        w.cnt = std::min(chunk, count - i0);
        w.i0 = f == 2 ? i0 : 0;
        w.aux0 = 3 * H->n_junctions;
        w.aux1 = H->off_base_ang;
        w.inv_t_swing = H->inv_t_swing;
        b.lists.fam[f].push_back(w);
      }
    };
    add(0, H->n_terrain_rows, H->o_terrain_rows, sizeof(TerrainRow), H->row_terrain, 1, H->nnz_terrain, 3);
    add(1, H->n_force_nodes, H->o_force_nodes, sizeof(ForceNode), H->row_force, 5, H->nnz_force, 25);
    add(2, 6 * H->n_junctions, H->o_acc, sizeof(AccJunction), H->row_acc, 1, H->nnz_acc, 6);
    add(3, H->n_swing_nodes, H->o_swing_nodes, sizeof(SwingNode), H->row_swing, 4, H->nnz_swing, 12);
  }
}
}  // namespace

BatchPlan PlanBatch(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem,
                    const std::vector<uint64_t>& blob_at, int n_cu, int64_t cache_bytes, int force_chunk) {
  BatchInputs in{structs, struct_of_problem, blob_at, {}, {}, {}};
  BatchPlan b;
  ShareLayouts(in, b);
  PlaceProblems(in, b);        // (checks struct_of_problem: everything below indexes with it)
  AddSliceItems(in, b);
  AddPhaseItems(in, b);
  AddFlatGroups(in, b);
  DecidePolicy(in, b, cache_bytes);
  OrderFlatGroups(in, b);      // (after the policy: a problem's score slots count node_families node waves)
  AddFamilyChunks(in, b, n_cu, force_chunk);
  return b;
}

// ---------------------------------------------------------------- twr_batch_start (start_table.h)
StartPlan PlanStart(const std::vector<const std::vector<char>*>& table_of_struct, const std::vector<int32_t>& struct_of_problem,
                    const std::vector<int64_t>& x_off, const std::vector<uint64_t>& blob_of_problem) {
  const size_t n_problems = struct_of_problem.size();
  if (x_off.size() != n_problems + 1 || blob_of_problem.size() != n_problems) throw std::runtime_error("PlanStart: list sizes");
  StartPlan plan;
  // every distinct table once, on a 256-byte line (a bucket per size and first words: equality is decided by memcmp)
  std::unordered_map<std::string, uint64_t> placed;
  std::vector<uint64_t> off_of_struct(table_of_struct.size());
  for (size_t i = 0; i < table_of_struct.size(); ++i) {
    if (!table_of_struct[i] || table_of_struct[i]->size() < sizeof(StartHeader)) throw std::runtime_error("PlanStart: structure without a start table");
    const std::vector<char>& t = *table_of_struct[i];
    plan.bytes_built += (int64_t)t.size();
    const auto at = placed.emplace(std::string(t.data(), t.size()), (uint64_t)plan.tables.size());
    if (at.second) {
      plan.tables.insert(plan.tables.end(), t.begin(), t.end());
      plan.tables.resize((plan.tables.size() + 255) / 256 * 256, 0);
      plan.bytes_distinct += (int64_t)t.size();
    }
    off_of_struct[i] = at.first->second;
  }
  for (size_t p = 0; p < n_problems; ++p) {
    const int32_t s = struct_of_problem[p];
    if (s < 0 || (size_t)s >= table_of_struct.size()) throw std::runtime_error("PlanStart: structure index out of range");
    const StartHeader& h = *reinterpret_cast<const StartHeader*>(plan.tables.data() + off_of_struct[s]);
    if (x_off[p + 1] - x_off[p] != h.n_vars) throw std::runtime_error("PlanStart: x offsets do not match the structure's variables");
    for (int v0 = 0; v0 < h.n_vars; v0 += kStartItem)
      plan.work.push_back({off_of_struct[s], blob_of_problem[p], x_off[p], v0, std::min(kStartItem, h.n_vars - v0), (int32_t)p, 0});
  }
  return plan;
}
void StartPlan::Place(uint64_t base) {
  for (StartWork& w : work) w.table += base;
}

EvalCounts CountsOf(const BatchPlan& P) {
  const BatchPlan::Lists& L = P.lists;
  EvalCounts c;
  c.dyn = (int)L.dyn.size(), c.rom = (int)L.rom.size(), c.node = std::max(0, (int)L.node.size() - 1), c.flat = (int)L.flat.size();
  for (int f = 0; f < 4; ++f) c.fam[f] = (int)L.fam[f].size();
  c.pdyn = (int)L.pdyn.size(), c.ploc = (int)L.ploc.size(), c.prom = (int)L.prom.size();
  return c;
}

EvalShape MakeEvalShape(const BatchPlan& P, const EvalCounts& c, int n_cu, int flags, bool events, const LaunchTuning& tuning) {
  const bool scoring = flags & kEvalScores;
  EvalShape s;
  s.n_cu = n_cu;
  s.dyn = c.dyn, s.rom = c.rom, s.node = c.node, s.flat = c.flat, s.pdyn = c.pdyn, s.ploc = c.ploc, s.prom = c.prom;
  for (int f = 0; f < 4; ++f) s.fam[f] = c.fam[f];
  s.rom_max_vals = P.rom_max_vals, s.flat_max_x = P.flat_max_x, s.dyn_map_chunks = P.dyn_map_chunks, s.node_families = P.node_families;
  s.pdyn_img_cap = P.pdyn_img_cap, s.prom_img_cap = P.prom_img_cap, s.stream_nt = P.stream_nt;
  if (!scoring) s.dyn_uniform = P.dyn_uniform;
  s.flags = scoring ? flags & (kEvalScores | kEvalBest) : flags & 3;
  s.events = events && !scoring;
  s.score_fused = scoring && P.score_fused;
  s.tuning = tuning;
  return s;
}

}  // namespace twr
