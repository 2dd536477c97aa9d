"""The case table of tests/test_style_kernels_gpu.py against csrc/vts_spade.hip, vts_style.hip, vts_style_levels.hip and the modconv entries
of vts_stylegan2.hip: every __global__ kernel behind the judged entries and every instance string of theirs is claimed by a row, no row claims
a string the source lacks, both sides of every dispatch, every chunk plan, cap, tail wavefront and second sweep have a row (computed from
the shapes with the plan formulas the table restates, which are held against the source text), the kink margins and planted zeros are what
the table says, and the derived units are honest: an fp32 torch evaluation of each header formula, in two summation orders, stays within
1.0 unit of the float64 judge on every row, a reference moved by 3 units at one element is rejected, and so are deliberately wrong fp32
restatements (biased or one-pass AdaIN variance, a corner of the class table treated as an edge, demodulation without eps, the power
iteration with u before v, the batch-grouped modulate backward grouped per plane, a scale_dot that drops its last chunk)."""
import os
import re

import pytest
import torch

import style_kernel_cases as T
from oracle import launch_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visual-tactile-synthesis_amd", "csrc")
FILES = {"vts_spade.hip": ["vts_spade_modulate", "vts_spade_modulate_bwd", "vts_spade_eval_stats", "vts_spectral_norm", "vts_spectral_norm_bwd"],
         "vts_style.hip": ["vts_adain", "vts_adain_bwd"],
         "vts_style_levels.hip": ["vts_style_bias", "vts_style_bias_bwd", "vts_style_linear", "vts_style_linear_bwd"],
         "vts_stylegan2.hip": ["vts_modconv_demod", "vts_modconv_demod_bwd", "vts_modconv_scale_dot", "vts_modconv_transpose", "vts_modconv_weight",
                               "vts_modconv_weight_bwd"]}
# kernels of the files that belong to entries judged elsewhere (tests/resample_cases.py)
ELSEWHERE = {"tanh_bwd_kernel", "nearest_fwd_kernel", "nearest_bwd_kernel", "nearest_up2_kernel", "nearest_up2_bwd_kernel", "upfirdn2d_kernel",
             "ufd_tile_kernel", "upfirdn2d_adj_kernel", "bias_act_kernel", "bias_act_bwd_kernel"}
BOUND = 1.01


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def global_kernels(text):
    return set(re.findall(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(", text))


def instance_strings(text):
    out = []
    for call in re.findall(r"\bvts_set_kernel\(([^;]*)\);", text):
        found = re.findall(r'"([^"]*)"', call)
        assert found, call
        out += found
    return set(out)


def entry_body(name, text):
    m = re.search(r'extern "C" int %s\(.*?\n}\n' % name, text, re.S)
    assert m, name
    return m.group(0)


def entry_instances():
    return {name: instance_strings(entry_body(name, source(f))) for f, names in FILES.items() for name in names}


# ---------------------------------------------------------------------------------------------------------------- table against the sources
def test_the_sources_are_read_as_expected():
    k = set().union(*(global_kernels(source(f)) for f in FILES))
    assert len(k) == 45 and {"spade_mod_bwd_sums", "adain_bwd_kernel", "style_dv_kernel", "scale_dot_finish_kernel", "wtranspose_kernel"} <= k, sorted(k)
    named = entry_instances()
    assert "scale_dot_rows_kernel<16,vec>" in named["vts_modconv_scale_dot"] and "spade_mod_bwd_sums<block> frozen" in named["vts_spade_modulate_bwd"]


def test_every_entry_names_its_instance_and_every_string_is_claimed():
    claimed = T.claimed_instances()
    for name, named in entry_instances().items():
        assert named, "%s does not call vts_set_kernel" % name
        assert named <= claimed, "%s: instances without a row in tests/style_kernel_cases.py: %s" % (name, sorted(named - claimed))


def test_every_row_claims_a_string_the_source_names():
    named = set().union(*entry_instances().values())
    assert T.claimed_instances() <= named, sorted(T.claimed_instances() - named)


def test_every_kernel_behind_the_entries_is_claimed_by_a_row():
    names = set().union(*(T.kernels_of(c) for c in T.claimed_instances()))
    for f in FILES:
        missing = global_kernels(source(f)) - ELSEWHERE - names
        assert not missing, "%s: __global__ kernels without a row in tests/style_kernel_cases.py: %s" % (f, sorted(missing))
    assert names <= set().union(*(global_kernels(source(f)) for f in FILES)), names


def test_the_restated_plans_are_those_of_the_sources():
    sp, sl, sg = source("vts_spade.hip"), source("vts_style_levels.hip"), source("vts_stylegan2.hip")
    assert "constexpr int kMaxBlocks = 4096;" in sp and T.GRID_CAP == 4096 * 256
    assert "if (out_pad == 0 && ((H * W) & 3) == 0 && aligned16(x, gamma, beta, out))" in sp
    assert "const bool wave = H * W <= 1024;" in sp and "const bool v4 = ((H * W) & 3) == 0 && aligned16(x, dx);" in sp
    assert "constexpr int kSnRows = 64;" in sp and "return (int64_t)cdiv(Co, kSnRows) * K + Co;" in sp
    assert "const int vec = (int)((K & 3) == 0 && aligned16(w, v));" in sp and "const int gx = cdiv(K, 256) < 16 ? cdiv(K, 256) : 16;" in sp
    assert "return 6ll * N * C;" in sp
    assert "constexpr int KSPLIT = 4;" in sl and "constexpr int MAX_CHUNKS = 64;" in sl
    assert "inline int row_chunks(int OH) { return min(max(cdiv(OH, 16), 1), MAX_CHUNKS); }" in sl
    assert "const int gx = (int)min((int64_t)256, cdiv64((int64_t)OH * OW, 2048));" in sl
    assert "inline int linear_chunks(int P) { return min(max(cdiv(P, 256), 1), 512); }" in sl
    assert "return (int64_t)N * Cout * 16 * (row_chunks(OH) + 1);" in sl
    assert "constexpr int SD_ROW_MAX = 1024, SD_CHUNK_MIN = 2048, SD_TARGET_WGS = 2048;" in sg
    assert "const bool narrow = HW <= (vec ? 256 : 64);" in sg and "const int CT = 256 / KK" in sg
    assert "const int64_t c = cdiv64(cdiv64(HW, s), 4) * 4;" in sg


def test_both_sides_of_every_dispatch_have_rows():
    # modulate: both instances; the scalar one by each single cause
    assert {T.mod_instance(r) for r in T.MOD} == {T.V4, T.PAD}
    causes = [(r[6] == 1, (r[3] * r[4]) % 4 != 0, r[7]) for r in T.MOD if T.mod_instance(r) == T.PAD]
    assert (True, False, None) in causes and (False, True, None) in causes
    assert {c[2] for c in causes if not c[0] and not c[1]} == {"x", "gamma", "beta", "out"}
    assert {(r[3], r[4]) for r in T.MOD} >= {(1, 1), (1, 7), (7, 1)} and {r[5] for r in T.MOD} == {T.ACT_NONE, T.ACT_LRELU}
    for inst in (T.V4, T.PAD):
        assert any(T.mod_instance(r) == inst and T.mod_work(r) > T.GRID_CAP for r in T.MOD), inst
        assert {r[5] for r in T.MOD if T.mod_instance(r) == inst} == {T.ACT_NONE, T.ACT_LRELU}
    # modulate backward
    assert {T.modb_instance(r) for r in T.MODB} == {s for s in T.claimed_instances() if s.startswith("spade_mod_bwd")} and len({T.modb_instance(r) for r in T.MODB}) == 6
    hw = {(r[3] * r[4], r[1] * r[2]) for r in T.MODB}
    assert {(1024, 1), (1024, 5), (1025, 1), (1025, 5)} <= hw
    assert {r[5] for r in T.MODB} == {0, 1, 2} and all(r[1] == 3 for r in T.MODB if r[5] == 1)
    assert {(r[8], r[3] * r[4] <= 1024) for r in T.MODB if r[5] == 2} == {("null", True), ("null", False), ("given", True), ("given", False)}
    assert all(r[8] == "own" for r in T.MODB if r[5] != 2) and {r[7] for r in T.MODB} == {0, 1}
    scalar = [((r[3] * r[4]) % 4 != 0, r[9]) for r in T.MODB if r[5] != 2 and not T.modb_instance(r).endswith("_v4")]
    assert (True, None) in scalar and (False, "x") in scalar and (False, "dx") in scalar
    for v4 in (True, False):
        assert any(T.modb_instance(r).endswith("_v4") == v4 and r[5] != 2 and T.modb_apply_work(r) > T.GRID_CAP for r in T.MODB), v4
    assert any(r[3] * r[4] == 1 and r[5] == 0 for r in T.MODB) and {r[10] for r in T.MODB} == {"own", "other"}
    # eval statistics: one workgroup, a full one, a second one
    assert {r[1] * r[2] for r in T.EVS} == {1, 256, 257}
    # spectral norm
    assert {(r[1], r[2]) for r in T.SN if r[3]} >= {(co, k) for co in T.SN_CO for k in T.SN_K}
    assert {T.sn_instance(r) for r in T.SN} == {s for s in T.claimed_instances() if "sn_wv_kernel" in s} and len({T.sn_instance(r) for r in T.SN}) == 4
    for training in (0, 1):
        sc = [(r[2] % 4 != 0, r[4]) for r in T.SN if r[3] == training and "scalar" in T.sn_instance(r)]
        assert any(c[0] and c[1] is None for c in sc) and (False, "w") in sc and (False, "v") in sc, training
    assert {cdiv_rows for cdiv_rows in {T.cdiv(r[1], 64) for r in T.SN}} == {1, 2, 3} and any(r[2] > 1024 for r in T.SN)
    assert {(r[1], r[2]) for r in T.SNB} >= {(co, k) for co in T.SN_CO for k in T.SN_K} and {r[3] for r in T.SNB} == {0, 1}
    assert {r[3] for r in T.SNB if T.snb_columns_stride(r[2])} == {0, 1}
    # AdaIN: tail wavefronts (NC % 4), the lane loop below, at and above 64 and 128
    assert {(r[1], r[2]) for r in T.ADA if r[3] == "plain"} == {(nc, hw) for nc in (1, 4, 5) for hw in (2, 36, 63, 64, 65, 129)}
    assert {r[3] for r in T.ADA} == {"plain", "offset", "scales"}
    # style bias
    for rows in (T.SB, T.SBB):
        assert {(r[4], r[5]) for r in rows} >= {(2, 2), (2, 4), (4, 2), (4, 4), (6, 10), (34, 62)}
        assert {r[2] for r in rows} == set(T.SB_K) and {r[3] for r in rows} == set(T.SB_COUT) and {r[7] for r in rows} == {"dense", "slice"}
        assert {r[6] for r in rows} == ({T.ACT_NONE, T.ACT_TANH} if rows is T.SB else {0, 1})
        assert {r[6] for r in rows if r[7] == "slice"} == {r[6] for r in rows}
        assert any(r[5] == 2 for r in rows) and any(r[5] == 130 for r in rows)
    chunks = {(r[4], r[5]): T.sb_pixel_chunks(r[4], r[5]) for r in T.SB}
    assert chunks[(34, 62)][0] == 2 and chunks[(6, 10)][0] == 1
    assert any(gx > 1 and per % ow != 0 for (oh, ow), (gx, per) in chunks.items())                  # a chunk boundary inside a row
    assert chunks[(1024, 514)][0] == 256 and T.cdiv(1024 * 514, 2048) > 256                          # the cap
    plans = {r[4]: T.sb_row_chunks(r[4]) for r in T.SBB}
    assert plans[18][0] == 2 and plans[34][0] == 3 and plans[1026][0] == 64 and plans[1026][2] > 0 and T.cdiv(1026, 16) > 64
    assert all(p[2] == 0 for oh, p in plans.items() if oh != 1026)
    for rows in (T.SB, T.SBB):
        for r in rows:
            code = T.sb_code(r).view(-1)
            assert code.numel() < 3 or (float(code[1]) == 0 and str(float(code[1])) == "0.0" and str(float(code[2])) == "-0.0" ), r[0]
        assert sum(1 for r in rows if r[1] * r[2] >= 6 and bool((T.sb_code(r) < 0).any())) >= 10
    # style Linear
    assert {r[3] for r in T.LIN if r[2] == 2} == set(T.LIN_P) and {r[2] for r in T.LIN if r[3] == 5} >= set(T.LIN_K) and {r[1] for r in T.LIN} == {1, 3}
    assert {T.lin_chunks(p)[0] for p in T.LIN_P} >= {1, 2, 512} and T.cdiv(131073, 256) > 512
    for dx in (0, 1):
        assert {r[5] for r in T.LINB if r[4] == dx} == {0, 1}
        assert {r[3] for r in T.LINB if r[4] == dx} >= {1, 257, 131073} if dx else True
    # modconv
    assert {r[3] * r[4] for r in T.DEM} == {1, 27, 256, 261} and {r[4] for r in T.DEM} == {1, 9, 16} and {r[2] for r in T.DEM} == {1, 5} and {r[1] for r in T.DEM} == {1, 3}
    assert {(r[4], r[5]) for r in T.MODWB} == {(0, 0), (0, 1), (1, 0), (1, 1)} and {r[4] for r in T.MODW} == {0, 1}
    assert {r[4] for r in T.DMB} >= {1, 9, 129, 256} and {T.dmb_tile(kk) for kk in (1, 9, 129, 256)} == {256, 28, 1}
    assert {r[3] for r in T.DMB if r[4] == 9} >= {28, 29} and {r[3] for r in T.DMB if r[4] == 1} >= {256, 257}
    assert any(r[2] % 4 for r in T.DMB) and {(r[5], r[6]) for r in T.DMB} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    inst = {T.sd_instance(r) for r in T.SD}
    assert inst == {s for s in T.claimed_instances() if s.startswith("scale_dot")} and len(inst) == 8
    by = {(r[2], T.sd_instance(r)) for r in T.SD}
    assert {(256, "scale_dot_rows_kernel<16,vec>"), (260, "scale_dot_rows_kernel<64,vec>"), (64, "scale_dot_rows_kernel<16,scalar>"),
            (65, "scale_dot_rows_kernel<64,scalar>"), (1024, "scale_dot_rows_kernel<64,vec>"), (1028, "scale_dot_split_kernel<vec>")} <= by
    ragged = {(r[1], r[2]): T.sd_plan(r[1], r[2]) for r in T.SD if r[2] > 1024}
    assert all(s == 1 or hw % c != 0 or nc == 1025 for (nc, hw), (c, s) in ragged.items())
    assert ragged[(3, 2049)][1] == 2 and ragged[(1, 4100)][1] == 3 and ragged[(1025, 4100)][1] == 2
    assert all(T.sd_ws_floats(r[1], r[2]) == (r[1] * ragged[(r[1], r[2])][1] if r[2] > 1024 and ragged[(r[1], r[2])][1] > 1 else 0) for r in T.SD)
    assert {r[4] for r in T.SD} == {None, "a", "b", "out"} and {r[3] for r in T.SD} == {0, 1} and {r[5] for r in T.SD} == {0, 1}
    for g in (16, 64):
        assert {r[1] % (256 // g) != 0 for r in T.SD if "rows_kernel<%d" % g in T.sd_instance(r)} == {True} and \
            {r[1] for r in T.SD if "rows_kernel<%d" % g in T.sd_instance(r)} >= {1, 17}
    assert {r[4] for r in T.TR} == {0, 1}
    for r in T.TR:
        for t in T.tr_inputs(r):
            assert bool(torch.equal(t * 1024, torch.round(t * 1024))) and float(t.abs().max()) <= 4


def test_row_ids_are_unique_and_operands_stay_small():
    ids = T.row_ids()
    assert len(ids) == len(set(ids)) and len(ids) > 200
    cap = 2 ** 22 + 10000
    assert all(r[1] * r[2] * r[3] * r[4] <= cap for r in T.MOD + T.MODB) and all(r[1] * r[2] <= cap for r in T.SD)
    assert all(r[1] * r[3] * r[4] * r[5] <= cap for r in T.SB + T.SBB) and all(r[1] * r[2] <= cap for r in T.SN + T.SNB)


# ---------------------------------------------------------------------------------------------------------------- kinks and planted zeros
@pytest.mark.parametrize("rows", [T.MOD, T.MODB], ids=["modulate", "modulate_bwd"])
def test_kink_margins_and_planted_zeros(rows):
    planted = 0
    for row in rows:
        lrelu = row[5 if rows is T.MOD else 6] == T.ACT_LRELU
        x, mean, rstd, gamma, beta, plant = (T.mod_inputs(row) if rows is T.MOD else T.modb_inputs(row)[1:])
        n, c = x.shape[:2]
        assert bool(plant.any()) == (lrelu and x.numel() > 3), row[0]
        if not lrelu:
            continue
        for dt in (torch.float64, torch.float32):
            t = (x.to(dt) - mean.to(dt).view(n, c, 1, 1)) * rstd.to(dt).view(n, c, 1, 1) * (1 + gamma.to(dt)) + beta.to(dt)
            assert bool((t[plant] == 0).all()) and bool((t[~plant].abs() >= 2 * T.KINK).all()), row[0]
        planted += int(plant.sum())
    assert planted >= 100


# ---------------------------------------------------------------------------------------------------------------- the fp32 arithmetic
class F32:
    """the arithmetic of the judges' formulas in plain fp32 torch; order 0: torch.sum, order 1: one term after the other, last term first"""

    def __init__(self, v, order):
        self.v, self.order = v, order

    @staticmethod
    def lifter(order):
        return lambda t: F32(t.detach().to(torch.float32), order)

    @property
    def val(self):
        return self.v

    def _co(self, o):
        return o.v if isinstance(o, F32) else torch.tensor(float(o), dtype=torch.float32)

    def __add__(self, o):
        return F32(self.v + self._co(o), self.order)

    __radd__ = __add__

    def __sub__(self, o):
        return F32(self.v - self._co(o), self.order)

    def __mul__(self, o):
        return F32(self.v * self._co(o), self.order)

    __rmul__ = __mul__

    def __truediv__(self, o):
        return F32(self.v / self._co(o), self.order)

    def __rtruediv__(self, o):
        return F32(self._co(o) / self.v, self.order)

    def sqrt(self):
        return F32(self.v.sqrt(), self.order)

    def rsqrt(self):
        return F32(self.v.rsqrt(), self.order)

    def tanh(self):
        return F32(self.v.tanh(), self.order)

    def sum(self, dim, keep=False, cnt=None):
        dim = (dim,) if isinstance(dim, int) else tuple(dim)
        if self.order == 0:
            return F32(self.v.sum(dim, keepdim=keep), self.order)
        rest = [d for d in range(self.v.dim()) if d not in dim]
        t = self.v.permute(rest + list(dim)).reshape([self.v.shape[d] for d in rest] + [-1]).flip(-1).cumsum(-1)[..., -1]
        if keep:
            t = t.reshape([1 if d in dim else self.v.shape[d] for d in range(self.v.dim())])
        return F32(t, self.order)

    def clamp_min(self, c):
        return F32(self.v.clamp_min(c), self.order)

    def mask(self, m):
        return F32(self.v * m.to(torch.float32), self.order)

    def slope(self, f, rounds):
        return F32(self.v * f.to(torch.float32), self.order)

    def map(self, fn):
        return F32(fn(self.v), self.order)


def _acc(t, on):
    return t if on else None


def judged_calls(table, row):
    """[(name, judge function taking A)] of a row: what tests/test_style_kernels_gpu.py judges, the later stages of the staged calls at
    the earlier stage's float64 value rounded to fp32"""
    f32 = lambda pair: pair[0].float()
    if table == "MOD":
        x, mean, rstd, gamma, beta, _ = T.mod_inputs(row)
        return [("out", lambda A: R.spade_modulate(x, mean, rstd, gamma, beta, row[5], row[6], A=A))]
    if table == "MODB":
        g, x, mean, rstd, gamma, beta, _ = T.modb_inputs(row)
        return [("bwd", lambda A: R.spade_modulate_bwd(g, x, mean, rstd, gamma, beta, row[5], row[6], A=A))]
    if table == "EVS":
        rm, rv = T.evs_inputs(row)
        return [("stats", lambda A: R.spade_eval_stats(rm, rv, T.EVS_EPS, row[1], A=A))]
    if table == "SN":
        w, u, v = T.sn_inputs(row)
        calls = []
        if row[3]:
            v = f32(R.spectral_norm_v(w, u, T.SN_EPS)["v"])
            calls.append(("v", lambda A: R.spectral_norm_v(w, u, T.SN_EPS, A=A)))
            calls.append(("u", lambda A: R.spectral_norm_u(w, v, T.SN_EPS, A=A)))
            u = f32(R.spectral_norm_u(w, v, T.SN_EPS)["u"])
        sigma = f32(R.spectral_norm_sigma(w, u, v)["sigma"])
        return calls + [("sigma", lambda A: R.spectral_norm_sigma(w, u, v, A=A)), ("scale", lambda A: R.spectral_norm_scale(w, sigma, A=A))]
    if table == "SNB":
        g, wsn, u, v, sg, dw0 = T.snb_inputs(row)
        total = f32(R.spectral_norm_bwd_total(g, wsn)["total"])
        return [("total", lambda A: R.spectral_norm_bwd_total(g, wsn, A=A)),
                ("dw", lambda A: R.spectral_norm_bwd_dw(g, total, u, v, sg, _acc(dw0, row[3]), A=A))]
    if table == "ADA":
        g, x, s = T.ada_inputs(row)
        return [("fwd", lambda A: R.adain(x, s, T.ADA_EPS, A=A)), ("bwd", lambda A: R.adain_bwd(g, x, s, T.ADA_EPS, A=A))]
    if table == "SB":
        code, w, out0 = T.sb_inputs(row)
        return [("out", lambda A: R.style_bias(code, w, out0, row[6], A=A))]
    if table == "SBB":
        g, code, dw0 = T.sbb_inputs(row)
        return [("dw", lambda A: R.style_bias_bwd(g, code, None, _acc(dw0, row[6]), A=A))]
    if table == "LIN":
        x, w, _, _ = T.lin_inputs(row)
        return [("z", lambda A: R.style_linear(x, w, A=A))]
    if table == "LINB":
        x, w, dz, dw0 = T.lin_inputs(row)
        return [("bwd", lambda A: R.style_linear_bwd(dz, x, w, _acc(dw0, row[5]), bool(row[4]), A=A))]
    if table == "DEM":
        w, s = T.dem_inputs(row)
        return [("demod", lambda A: R.modconv_demod(w, s, T.mod_scale(row[3], row[4]), T.DEM_EPS, A=A))]
    if table == "MODW":
        w = T.modw_inputs(row)[0]
        return [("wout", lambda A: R.modconv_weight(w, T.mod_scale(row[2], row[3]), T.DEM_EPS, row[4], A=A))]
    if table == "MODWB":
        w, g, dw0 = T.modw_inputs(row)
        return [("dw", lambda A: R.modconv_weight_bwd(w, g, T.mod_scale(row[2], row[3]), T.DEM_EPS, row[4], _acc(dw0, row[5]), A=A))]
    if table == "DMB":
        dd, d, w, s, dw0, ds0 = T.dmb_inputs(row)
        return [("bwd", lambda A: R.modconv_demod_bwd(dd, d, w, s, T.mod_scale(row[3], row[4]), _acc(dw0, row[5]), _acc(ds0, row[6]), A=A))]
    if table == "SD":
        a, b, f, dot0 = T.sd_inputs(row)
        return [("dot", lambda A: R.modconv_scale_dot(a, b, f, T.SD_ALPHA, bool(row[3]), _acc(dot0, row[5]), A=A))]
    assert table == "TR"
    w, o0 = T.tr_inputs(row)
    return [("out", lambda A: R.modconv_transpose(w, _acc(o0, row[4]), A=A))]


ROWS = [(name, row) for name, rows in T.TABLES.items() for row in rows]


@pytest.mark.parametrize("table,row", ROWS, ids=[r[0] for _, r in ROWS])
def test_units_are_honest_on_every_row(table, row):
    """fp32 in two summation orders within 1.0 unit; every unit finite and nonnegative; a reference moved by 3 units at one element rejected"""
    for name, fn in judged_calls(table, row):
        ref = fn(None)
        for order in (0, 1):
            got = fn(F32.lifter(order))
            assert set(got) == set(ref)
            for k, (r, unit) in ref.items():
                assert r.shape == got[k].shape and bool(torch.isfinite(unit).all()) and bool((unit >= 0).all()) and bool(torch.isfinite(r).all()), (row[0], name, k)
                ratio, at = R.worst(got[k], r, unit)
                assert ratio <= 1.0, "%s %s %s order %d: fp32 is %.3f units off at element %d" % (row[0], name, k, order, ratio, at)
        for k, (r, unit) in ref.items():
            i = int(torch.argmax(unit.reshape(-1)))
            if float(unit.reshape(-1)[i]) == 0:
                continue                     # an exact output: bitwise in the GPU test
            moved = r.clone().reshape(-1)
            moved[i] += 3 * unit.reshape(-1)[i]
            assert R.worst(r, moved.reshape(r.shape), unit)[0] > BOUND


# ---------------------------------------------------------------------------------------------------------------- wrong restatements
def rejected(got, pair):
    return R.worst(got, pair[0], pair[1])[0] > BOUND


def _row(rows, rid):
    return next(r for r in rows if r[0] == rid)


def _adain32(x, s, eps, biased=False, one_pass=False):
    m = x.shape[1]

    def stats(p):
        mean = p.sum(1, keepdim=True) / m
        if one_pass:
            var = ((p * p).sum(1, keepdim=True) - m * mean * mean) / (m - 1)
        else:
            var = ((p - mean) ** 2).sum(1, keepdim=True) / (m if biased else m - 1)
        return mean, (var + eps).sqrt()
    (mx, sx), (ms, ss) = stats(x), stats(s)
    return (x - mx) / sx * ss + ms


def test_adain_with_a_biased_or_a_one_pass_variance_is_rejected():
    # the factor m / (m - 1) cancels between the two stds unless eps counts: the row whose style map has a variance below eps
    g, x, s = T.ada_inputs(_row(T.ADA, "ada-scales-1e3-1e-3"))
    assert float(s.double().var(1).max()) < T.ADA_EPS
    ref = R.adain(x, s, T.ADA_EPS)["out"]
    assert not rejected(_adain32(x, s, T.ADA_EPS), ref) and rejected(_adain32(x, s, T.ADA_EPS, biased=True), ref)
    for rid in ("ada-offset-100-std", "ada-offset-100-std-hw129"):
        g, x, s = T.ada_inputs(_row(T.ADA, rid))
        assert abs(float((x.double().mean(1).abs() / x.double().std(1)).mean()) - 100) < 10
        ref = R.adain(x, s, T.ADA_EPS)["out"]
        assert not rejected(_adain32(x, s, T.ADA_EPS), ref), rid
    assert rejected(_adain32(x, s, T.ADA_EPS, one_pass=True), ref)


def _style_bias32(code, w, out0, corner_as_edge=False):
    """the header's class table: per axis {first, other even, other odd, last} reach kernel indices {1}, {1, 3}, {0, 2}, {2}"""
    taps = [(1,), (1, 3), (0, 2), (2,)]
    oh, ow = out0.shape[-2:]
    cls = lambda o, size: 0 if o == 0 else (3 if o == size - 1 else (2 if o % 2 else 1))
    V = torch.einsum("nc,cjyx->njyx", code.clamp_min(0), w)
    out = out0.clone()
    for oy in range(oh):
        for ox in range(ow):
            ry, rx = cls(oy, oh), cls(ox, ow)
            if corner_as_edge and oy == 0 and ox == 0:
                rx = 1
            out[:, :, oy, ox] += sum(V[:, :, ky, kx] for ky in taps[ry] for kx in taps[rx])
    return out


def test_the_class_table_with_a_corner_treated_as_an_edge_is_rejected():
    for rid in ("sb-6x10-k5-co5-none-dense", "sb-4x4-k4-co1-tanh-dense"):
        row = _row(T.SB, rid)
        code, w, out0 = T.sb_inputs(row)
        ref = R.style_bias(code, w, out0, T.ACT_NONE)["out"]
        assert not rejected(_style_bias32(code, w, out0), ref) and rejected(_style_bias32(code, w, out0, corner_as_edge=True), ref)


def test_demodulation_without_eps_is_rejected():
    row = _row(T.DEM, "dem-eps-matters")
    w, s = T.dem_inputs(row)
    sc = torch.tensor(T.mod_scale(row[3], row[4]), dtype=torch.float32)
    ref = R.modconv_demod(w, s, float(sc), T.DEM_EPS)["demod"]
    acc = sc * sc * ((w[None] * s[:, None, :, None]) ** 2).sum((2, 3))
    assert not rejected((acc + T.DEM_EPS).rsqrt(), ref) and rejected(acc.rsqrt(), ref)


def test_the_power_iteration_with_u_before_v_is_rejected():
    row = _row(T.SN, "sn-co65-k257-train")
    w, u, v = T.sn_inputs(row)
    unit = lambda t: t / t.norm().clamp_min(T.SN_EPS)
    ref = R.spectral_norm_v(w, u, T.SN_EPS)["v"]
    assert not rejected(unit(w.t() @ u), ref) and rejected(unit(w.t() @ unit(w @ v)), ref)


def test_the_batch_grouped_modulate_backward_grouped_per_plane_is_rejected():
    row = _row(T.MODB, "mb-mode1-wave")
    g, x, mean, rstd, gamma, beta, _ = T.modb_inputs(row)
    ref = R.spade_modulate_bwd(g, x, mean, rstd, gamma, beta, 1, row[6])["dx"]
    A = F32.lifter(0)
    assert not rejected(R.spade_modulate_bwd(g, x, mean, rstd, gamma, beta, 1, row[6], A=A)["dx"], ref)
    assert rejected(R.spade_modulate_bwd(g, x, mean, rstd, gamma, beta, 0, row[6], A=A)["dx"], ref)


def test_a_scale_dot_that_drops_its_last_chunk_is_rejected():
    for rid in ("sd-split-scalar-hw2049", "sd-split-vec-hw4100-nc1"):
        row = _row(T.SD, rid)
        a, b, f, dot0 = T.sd_inputs(row)
        chunk, s = T.sd_plan(row[1], row[2])
        ref = R.modconv_scale_dot(a, b, f, T.SD_ALPHA, False, _acc(dot0, row[5]))["dot"]
        dot = lambda upto: (dot0 if row[5] else 0) + torch.tensor(T.SD_ALPHA) * (a[:, :upto] * b[:, :upto]).sum(1)
        assert s > 1 and not rejected(dot(row[2]), ref) and rejected(dot((s - 1) * chunk), ref)
