"""The instantiation matrix of the evaluation kernels, stated once.

twr_batch_eval picks one template instantiation of each kernel from whole-batch quantities (batch_plan.cc PlanBatch /
eval_plan.cc PlanEval).  MATRIX below names small batches -- real shapes, nothing else -- that between them reach every instantiation
that can be planned, and says which ones each batch reaches.  Two readers build the same structures from this text:

  tests/eval_matrix_driver.cc (run by tests/test_eval_matrix_plan.py, no GPU) plans every row with the product's planner and
      checks the claims, and that claims + exclusions are exactly the instantiations that exist;
  tests/test_eval_matrix.py (GPU) runs every row and compares it with the oracle.

Format, one record per line, fields separated by blanks:

  struct NAME [robot=anymal] [terrain=flat|stairs|gap] [combo=1] [swing=1.0] [T=2.0] [K=40] [sets=27] [pps=2] [ppf=3] [dbp=0.1] [dbm=0.025]
      gait_combo(n_ee, combo, T, swing); dt_dynamic = dt_rom = T / (K - 1.5), i.e. K time nodes; sets = TWR_SET_* mask
      (27: terrain, dynamic, range of motion, force; 63: + splineacc, swing; +64: optimised phase durations); pps / ppf =
      polynomials per swing phase / per stance phase of the force; dbp = duration of a base polynomial; dbm = time step of the baseMotion set (sets & 128).
  row NAME kind=cheap|wide|chunk|nt structs=A,B*3 order=0,1,1|cycle:N [nt=1] [val_off=..] [val_on=..] [jac_off=..] [jac_on=..] [scores=..]
      structs: the batch's structure list (B*3: B three times -- three tables in the arena, three structure indices);
      order: struct_of_problem (cycle:N: problem p of N uses structure p modulo the list length);
      nt=1: the batch streams its Jacobian out with non-temporal stores;
      claims, ';'-separated instantiation names as Batch.eval_plan spells them: val_* for EVAL_VALUES, jac_* for EVAL_JACOBIAN
      and EVAL_BOTH, *_off without and *_on with per-kernel events, scores for eval_scores_device (eval_score_best_device:
      the same + best_kernel).  '*' stands for the store variant of the call: G, J or GJ, with NT appended for the dyn, rom and
      fused kernels of an nt=1 row when the call writes the Jacobian.
      kinds: cheap = at most 8 problems of K <= 200; wide = at most 8 problems of any K (one row: more than 2046 variables AND
      slices that stage <= 128 doubles need 400 time nodes); chunk = at least 8 problems per CU (node_chunk_kernel); nt = just
      over 256 MB of output with fewer than four problems per structure.
  exclude INSTANTIATION the rule of PlanBatch / PlanEval that forbids it for every batch
"""
import functools

import towr_amd as ta

MATRIX = """
# ---- structures (ANYmal unless said otherwise)
struct k40    K=40
struct k40s   K=40 terrain=stairs combo=0 T=2.4 swing=1.1
struct k52    K=52
struct k52s   K=52 terrain=stairs combo=0 T=2.4 swing=1.1
struct k52g   K=52 terrain=gap combo=2 T=1.8 swing=0.9
struct k120   K=120
struct k120s  K=120 terrain=stairs combo=0 T=2.4 swing=1.1
struct k160   K=160
struct k200   K=200
struct k200s  K=200 terrain=stairs combo=0 T=2.4 swing=1.1
struct k200g  K=200 terrain=gap combo=2 T=1.8 swing=0.9
struct k200a  K=200 sets=63 terrain=stairs
struct k200p3 K=200 pps=3
struct k200p3s K=200 pps=3 terrain=stairs combo=0 T=2.4 swing=1.1
struct t4     K=40 T=4.0
struct t8     K=40 T=8.0 terrain=gap
struct t16    K=20 T=16.0
struct t16b   K=24 T=16.0 terrain=stairs
struct w400   K=400 T=16.0
struct tt     K=40 sets=65
struct p40    K=40 sets=91
struct p40a   K=40 sets=127 terrain=stairs
struct p40p3  K=40 sets=91 pps=3
struct p40p4  K=40 sets=91 pps=4 terrain=gap
struct p40p6  K=40 sets=91 pps=6
struct bm40   K=40 sets=155 dbm=5.2e-6
struct bm200  K=200 sets=155 dbm=5.2e-6
struct c12    K=12 sets=63
struct c12s   K=12 sets=63 terrain=stairs combo=0 T=2.4
struct c12g   K=12 sets=63 terrain=gap combo=2 T=1.8

# ---- cheap rows: fixed timings, the values-only path on
row k40_two      kind=cheap structs=k40,k40s order=0,1,0,1,1 val_off=eval_values_kernel<3> val_on=eval_values_kernel<3>;node_kernel2 jac_off=eval_fused_kernel<34,xc4,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<26,*>;node_kernel2 scores=eval_scores_kernel<3>;score_fold_kernel
row k40_one      kind=cheap structs=k40 order=0,0,0 val_off=eval_values_kernel<3> jac_off=eval_fused_kernel<34,xc4,*> jac_on=dyn_uniform_kernel<*,xc4>;rom_kernel<26,*>;node_kernel2
row k120_one     kind=cheap structs=k120 order=0,0,0 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_uniform_kernel<*,xc2>;rom_kernel<30,*>
row k160_one     kind=cheap structs=k160 order=0,0,0 jac_off=eval_fused_kernel<38,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<38,*>
row k200_two     kind=cheap structs=k200,k200a order=0,1,0 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<34,*>;node_kernel val_on=eval_values_kernel<3>;node_kernel
row k200_one     kind=cheap structs=k200 order=0,0,0 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_uniform_kernel<*,xc2>;rom_kernel<34,*>
row k200p3_k40   kind=cheap structs=k200p3,k40 order=0,1,1 jac_off=eval_fused_kernel<38,xc4,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<38,*>
row k200p3_one   kind=cheap structs=k200p3 order=0,0 jac_off=eval_fused_kernel<38,xc2,*> jac_on=dyn_uniform_kernel<*,xc2>;rom_kernel<38,*>
row t4_one       kind=cheap structs=t4 order=0,0 val_off=eval_values_kernel<5> val_on=eval_values_kernel<5> scores=eval_scores_kernel<5>;score_fold_kernel
row t8_two       kind=cheap structs=t8,k40 order=0,1,0 val_off=eval_values_kernel<8> val_on=eval_values_kernel<8> scores=eval_scores_kernel<8>;score_fold_kernel
# ---- cheap rows: more than 2046 variables (T = 16 s), the values-only path off
row t16_one      kind=cheap structs=t16 order=0,0,0 val_off=eval_fused_kernel<34,xc4,*> val_on=dyn_uniform_kernel<*,xc4>;rom_kernel<26,*>;node_kernel2 jac_off=eval_fused_kernel<34,xc4,*> scores=eval_fused_kernel<34,xc4,G>;score_kernel
row t16_two      kind=cheap structs=t16,t16b order=0,1,1 val_off=eval_fused_kernel<34,xc4,*> val_on=dyn_kernel<*,xc4>;rom_kernel<26,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<26,*>
row t16_k200p3   kind=cheap structs=t16,k200p3 order=0,1 val_off=eval_fused_kernel<38,xc4,*> val_on=dyn_kernel<*,xc4>;rom_kernel<38,*> jac_off=eval_fused_kernel<38,xc4,*>
# ---- cheap rows: a problem with optimised timings but neither dynamic nor range-of-motion rows switches the values-only path off
# and leaves the fused launch on
row k200_tt      kind=cheap structs=k200,tt order=0,1,0 val_off=eval_fused_kernel<34,xc2,*> val_on=dyn_kernel<*,xc2>;rom_kernel<34,*>;node_kernel jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<34,*> scores=eval_fused_kernel<34,xc2,G>;score_kernel
row k200p3_tt    kind=cheap structs=k200p3,tt order=0,1 val_off=eval_fused_kernel<38,xc2,*> val_on=dyn_kernel<*,xc2>;rom_kernel<38,*> jac_off=eval_fused_kernel<38,xc2,*>
row k120_tt      kind=cheap structs=k120,tt,k120s order=0,1,2 val_off=eval_fused_kernel<34,xc2,*> val_on=dyn_kernel<*,xc2>;rom_kernel<30,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<30,*>
# ---- cheap rows: optimised timings (the phase kernels), alone and beside fixed timings
row p40_two      kind=cheap structs=p40,p40a order=0,1,0 val_off=phase_locate_kernel;dyn_phase_kernel<40,*>;rom_phase_kernel<24,*>;node_kernel jac_off=phase_locate_kernel;dyn_phase_kernel<40,*>;rom_phase_kernel<24,*>;node_kernel jac_on=dyn_phase_kernel<40,*>;rom_phase_kernel<24,*> scores=dyn_phase_kernel<40,G>;rom_phase_kernel<24,G>;score_kernel
row p40p3_one    kind=cheap structs=p40p3 order=0,0 val_off=dyn_phase_kernel<0,*>;rom_phase_kernel<32,*> jac_off=dyn_phase_kernel<0,*>;rom_phase_kernel<32,*>
row p40p4_one    kind=cheap structs=p40p4 order=0,0 val_off=dyn_phase_kernel<0,*>;rom_phase_kernel<40,*> jac_off=dyn_phase_kernel<0,*>;rom_phase_kernel<40,*>
row p40p6_p40    kind=cheap structs=p40p6,p40 order=0,1,0 val_off=dyn_phase_kernel<0,*>;rom_phase_kernel<0,*> jac_off=dyn_phase_kernel<0,*>;rom_phase_kernel<0,*>
row p40_k40      kind=cheap structs=p40,k40,k40s order=0,1,2,0 val_off=dyn_kernel<*,xc4>;phase_locate_kernel;dyn_phase_kernel<40,*>;rom_phase_kernel<24,*>;rom_kernel<26,*>;node_kernel jac_off=dyn_kernel<*,xc4>;dyn_phase_kernel<40,*>;rom_phase_kernel<24,*>;rom_kernel<26,*>
# ---- wide row: one structure of more than 2046 variables whose slices stage <= 128 doubles
row w400_one     kind=wide structs=w400 order=0,0 val_off=eval_fused_kernel<38,xc2,*> val_on=dyn_uniform_kernel<*,xc2>;rom_kernel<38,*> jac_on=dyn_uniform_kernel<*,xc2>;rom_kernel<38,*>
# ---- chunk row: eight problems per CU, all four node families
row chunk_three  kind=chunk structs=c12,c12s,c12g order=cycle:2051 val_off=eval_values_kernel<3>;node_chunk_kernel<*> val_on=eval_values_kernel<3>;node_chunk_kernel<*> jac_off=eval_fused_kernel<34,xc4,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<26,*>;node_chunk_kernel<*>
# ---- nt rows: sweep-like batches writing just over the memory-side cache
row nt_k200      kind=nt nt=1 structs=k200*27,k200s*27,k200g*26 order=cycle:319 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<34,*>
row nt_k200p3    kind=nt nt=1 structs=k200p3*40,k200p3s*40 order=cycle:319 jac_off=eval_fused_kernel<38,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<38,*>
row nt_k52       kind=nt nt=1 structs=k52*110,k52s*110,k52g*110 order=cycle:1319 jac_off=eval_fused_kernel<34,xc4,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<26,*>
row nt_k200p3_k40 kind=nt nt=1 structs=k200p3*72,k40*33 order=cycle:419 jac_off=eval_fused_kernel<38,xc4,*> jac_on=dyn_kernel<*,xc4>;rom_kernel<38,*>
row nt_k120      kind=nt nt=1 structs=k120*65,k120s*65 order=cycle:519 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_kernel<*,xc2>;rom_kernel<30,*>

# ---- nt rows on ONE structure: three problems whose baseMotion set (a time node every 5.2 us) writes 92 MB each.  The only way
# into the non-temporal bodies of dyn_uniform_kernel: one structure index means at most three problems may stream
row nt_bm40      kind=nt nt=1 structs=bm40 order=0,0,0 jac_off=eval_fused_kernel<34,xc4,*> jac_on=dyn_uniform_kernel<*,xc4>;rom_kernel<26,*>;node_kernel
row nt_bm200     kind=nt nt=1 structs=bm200 order=0,0,0 jac_off=eval_fused_kernel<34,xc2,*> jac_on=dyn_uniform_kernel<*,xc2>;rom_kernel<34,*>;node_kernel

# ---- exclusions: none.  Every instantiation is reached by a row above.
"""


def _fields(tokens):
    return dict(t.split("=", 1) for t in tokens)


def parse(text=MATRIX):
    """(structs: name -> fields, rows: list of dicts, exclusions: instantiation -> rule)"""
    structs, rows, exclusions = {}, [], {}
    for line in text.splitlines():
        tok = line.split()
        if not tok or tok[0].startswith("#"):
            continue
        if tok[0] == "exclude":
            exclusions[tok[1]] = " ".join(tok[2:])
        elif tok[0] == "struct":
            structs[tok[1]] = _fields(tok[2:])
        elif tok[0] == "row":
            f = _fields(tok[2:])
            names = []
            for item in f["structs"].split(","):
                name, _, count = item.partition("*")
                names += [name] * int(count or 1)
            if f["order"].startswith("cycle:"):
                order = [p % len(names) for p in range(int(f["order"][6:]))]
            else:
                order = [int(o) for o in f["order"].split(",")]
            rows.append(dict(name=tok[1], kind=f.get("kind", "cheap"), nt=f.get("nt", "0") == "1", structs=names, order=order,
                             claims={k: [c for c in f.get(k, "").split(";") if c] for k in ("val_off", "val_on", "jac_off", "jac_on", "scores")}))
        else:
            raise ValueError("unknown line: " + line)
    return structs, rows, exclusions


_NT_KERNELS = ("dyn_kernel", "dyn_uniform_kernel", "rom_kernel", "eval_fused_kernel")


def claims_of(row, flags, events):
    """The instantiations the row claims for eval_device(flags) with / without per-kernel events, stores filled in."""
    store = {ta.EVAL_VALUES: "G", ta.EVAL_JACOBIAN: "J", ta.EVAL_BOTH: "GJ"}[flags]
    key = ("val" if flags == ta.EVAL_VALUES else "jac") + ("_on" if events else "_off")
    out = []
    for c in row["claims"][key]:
        nt = row["nt"] and (flags & ta.EVAL_JACOBIAN) and c.startswith(_NT_KERNELS)
        out.append(c.replace("*", store + ("NT" if nt else "")))
    return out


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The Case (product structure + oracle problem) of a `struct` line: the formulas of eval_matrix_driver.cc build()."""
    from tests.common import Case, k_params

    f = parse()[0][name]
    robot, terrain = f.get("robot", "anymal"), f.get("terrain", "flat")
    T, K = float(f.get("T", 2.0)), int(f.get("K", 40))
    model = ta.model_preset(robot, terrain)
    sched = ta.gait_combo(model.n_ee, int(f.get("combo", 1)), T, float(f.get("swing", 1.0)))
    return Case(robot, terrain, sched, duration_base_poly=float(f.get("dbp", 0.1)), polys_per_swing=int(f.get("pps", 2)),
                polys_per_stance_force=int(f.get("ppf", 3)), constraint_sets=int(f.get("sets", 27)), dt_base_motion=float(f.get("dbm", 0.025)),
                base_z_init=-model.nominal_stance[0][2], **k_params(T, K))
