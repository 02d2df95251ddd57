"""CPU tests (-m "not gpu") that pin the case table of the direct FIR kernel's GPU tests (tests/direct_fir_cases.py): the planner itself
-- tests/c/direct_plan_probe.cpp, a stand-alone host program that links csrc/xl_plan.cpp alone, built with ASan and UBSan and run as a
process of its own, as tests/test_plan_cpu.py builds plan_sweep.cpp -- must give every case x height the tile height, lane count, read
width, tap padding and tile fill the table names it for; the calls must hold the edges they are chosen for; and the sparse block of
test_sparse_block_is_exact_in_optimized_mode must have the single-term property its exactness rests on."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import direct_fir_cases as dc
from conftest import ROOT

CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "c", "direct_plan_probe.cpp"), os.path.join(CSRC, "xl_plan.cpp")]
CXX = shutil.which("g++") or "/opt/rocm/lib/llvm/bin/clang++"
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # (hip_runtime.h's types only: nothing of HIP is linked)
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ALL = [(case, H) for case in dc.CASES for H in dc.HEIGHTS]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """-> run(exp_h, max_samples, gcap, [(D, T, count, consumed)]) -> [launch dict] of the planner"""
    tmp = tmp_path_factory.mktemp("direct_plan_probe")
    objs = [str(tmp / (os.path.basename(s) + ".o")) for s in SOURCES]
    procs = [subprocess.Popen([CXX] + FLAGS + ["-I", CSRC, "-I", ROCM_INCLUDE, "-D__HIP_PLATFORM_AMD__", "-c", s, "-o", o],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s, o in zip(SOURCES, objs)]
    for p in procs:
        _, err = p.communicate()
        assert p.returncode == 0, err[-2000:]
    exe = str(tmp / "direct_plan_probe")
    r = subprocess.run([CXX, "-fsanitize=address,undefined"] + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def run(exp_h, max_samples, gcap, class_list):
        r = subprocess.run([exe, str(exp_h), str(max_samples), str(gcap)] + ["%d:%d:%d:%d" % tuple(c) for c in class_list],
                           capture_output=True, text=True, timeout=60)
        lines = r.stdout.splitlines()
        assert r.returncode == 0 and r.stderr == "" and lines and lines[-1].startswith("ok "), (r.stdout[-500:], r.stderr[-2000:])
        launches = []
        for ln in lines[:-1]:
            kind, rest = ln.split(" ", 1)
            f = dict(kv.split("=") for kv in rest.split())
            if kind == "launch":
                launches.append({k: int(v) for k, v in f.items()})
                launches[-1]["g"] = []
            else:
                g = {k: int(v) for k, v in f.items() if k != "tiles"}
                g["tiles"] = [int(v) for v in f["tiles"].split(",")]
                launches[-1]["g"].append(g)
        assert int(lines[-1].split()[1]) == len(launches)
        return launches

    return run


def _plan(probe, case, H, consumed=0):
    return probe(H, dc.max_input(case, H), dc.GROUP_BLOCKS, [(c.D, c.T, c.count, consumed) for c in dc.classes(case, H)])


def _claimed_wide(case, H):
    """whether the tall launch reads the window 16 bytes at a time (every decimation of the launch even)"""
    if case == "even":
        return H != 8  # (at 8 the class of six clients, D = 21, shares the launch)
    if case == "all_even":
        return True
    if case in ("odd_mixed", "short_taps"):
        return False
    return H in (8, 10)


def test_restated_constants_are_the_headers():
    grid = open(os.path.join(CSRC, "xl_grid.h")).read()
    dev = open(os.path.join(CSRC, "xl_device.h")).read()
    plan = open(os.path.join(CSRC, "xl_plan.cpp")).read()
    assert re.search(r"#define XL_HCAP (\d+)u", grid).group(1) == str(dc.XL_HCAP)
    assert re.search(r"#define XL_PH_STRIDE (\d+)u", grid).group(1) == str(dc.XL_PH_STRIDE)
    assert re.search(r"#define XL_NW_DEFAULT (\d+)", dev).group(1) == str(dc.XL_NW)
    assert "return (ct == 9 || ct == 10) ? 6u : 4u;" in dev
    assert "kHeights[XL_NLAUNCH] = {12, 10, 9, 8, 4, 2, 1}" in plan
    assert "#define XL_WIDE_LDS_BUDGET (160u * 1024u)" in open(os.path.join(CSRC, "xl_wide.h")).read()


@pytest.mark.parametrize("case,H", ALL, ids=lambda v: str(v))
def test_planner_gives_every_case_its_launch(probe, case, H):
    launches = {L["ct"]: L for L in _plan(probe, case, H)}
    cls = dc.classes(case, H)
    # ---- every shape is a narrow client inside the history
    for c in cls:
        assert not dc.needs_wide(c.D, c.T, 12) and c.T - 1 + c.D <= dc.XL_HCAP, c
    # ---- the table's claims about the tall launch: height, lanes, read width, tap padding, tile fill
    tall = launches[H]
    assert tall["ota"] == dc.LANES[case], (case, H, tall)
    assert tall["wide"] == int(_claimed_wide(case, H)), (case, H, tall)
    step = dc.tap_step(H)
    assert step == (6 if H in (9, 10) else 4)
    for g in tall["g"]:
        assert g["Tpad"] % step == 0 and g["Tpad"] == dc.roundup(g["T"], step) and g["rem0"] == 0, g
        assert g["hv0"] == (dc.XL_HCAP if g["T"] == 1 else 0), g  # (a single tap needs no history: mature from the start)
    tall_groups = [g for g in tall["g"] if (g["D"], g["T"]) == (cls[0].D, cls[0].T)]
    if case in ("even", "all_even", "odd_mixed"):  # five full tiles and one of three clients: two groups, the second with two spare waves
        assert [g["tiles"] for g in tall_groups] == [[H] * 4, [H, 3]], tall_groups
        assert tall["idle"] >= 2 and tall_groups[1]["ntiles"] == dc.XL_NW - 2
    else:  # a full tile and a tile of one client
        assert [g["tiles"] for g in tall_groups] == [[H, 1]], tall_groups
    if case == "even":  # heights 8, 4, 2, 1 beside it
        assert sorted(launches) == sorted({H, 8, 4, 2, 1}), sorted(launches)
        assert launches[8]["wide"] == 0 and launches[4]["wide"] == 0 and launches[2]["wide"] == 1 and launches[1]["wide"] == 0
    elif case == "all_even":  # ... every one of them with 16-byte reads at 64 lanes; at H = 8 three groups in the one h8 launch
        assert sorted(launches) == sorted({H, 8, 4, 2, 1}), sorted(launches)
        assert all(L["wide"] == 1 and L["ota"] == 64 for L in launches.values())
        assert launches[8]["groups"] == (3 if H == 8 else 1)
    else:
        assert sorted(launches) == [H], sorted(launches)
    if case == "odd_mixed":  # an even-D group in the same launch
        assert {g["D"] for g in tall["g"]} == {21, 42}
    if case == "short_taps":
        assert any(g["T"] < step for g in tall["g"]) and any(g["Tpad"] == step for g in tall["g"])  # below one step; steps / 2 == 0
        assert [g["Tpad"] for g in tall["g"]] == ([6, 6, 6, 12, 18] if step == 6 else [4, 8, 8, 8, 16])
    if case.startswith("lanes"):  # the D = 42 class runs at the short lane count too; the large decimation's parity follows H
        assert {g["D"] for g in tall["g"]} == {cls[0].D, 42} and cls[0].D % 2 == (1 if H in (9, 12) else 0)
        assert dc.lds_bytes(cls[0].D, dc.roundup(cls[0].T, step), 2 * tall["ota"]) > dc.LDS_BUDGET  # ... and no larger count fits
    # ---- the whole launch set is the restated one (the GPU test builds the expected describe() text from it)
    exp = dc.expected_launches([(c.D, c.T, c.count) for c in cls], H)
    assert sorted(exp) == sorted(launches)
    for ct, L in launches.items():
        e = exp[ct]
        assert (L["groups"], L["ota"], L["wide"]) == (e["groups"], e["ota"], int(e["wide"])), (ct, L, e)
        assert [g["tiles"] for g in L["g"]] == e["tiles"] and [g["Tpad"] for g in L["g"]] == e["tpads"], (ct, L, e)


def test_every_case_meets_every_format():
    for case in dc.CASES:
        assert sorted(dc.fmt_of(case, H) for H in dc.HEIGHTS) == sorted(dc.FMTS)
    for case in dc.SPARSE_CASES:
        assert all(dc.sparse_fmt_of(case, H) != "cu8" for H in dc.HEIGHTS)
        assert len({dc.sparse_fmt_of(case, H) for H in dc.HEIGHTS}) == 3


def test_clients_of_a_class_are_distinct():
    for case, H in ALL:
        cl = dc.clients(case, H)
        assert len(cl) == sum(c.count for c in dc.classes(case, H))
        for k, cs in enumerate(dc.classes(case, H)):
            mine = [(t.tobytes(), fc) for kk, D, t, fc in cl if kk == k]
            assert len({t for t, _ in mine}) == cs.count and len({fc for _, fc in mine}) == cs.count, (case, H, k)
            assert all(abs(fc) < dc.FS // 2 for _, fc in mine)
            assert all(len(t) == 4 * cs.T for t, _ in mine)


@pytest.mark.parametrize("case,H", ALL, ids=lambda v: str(v))
def test_call_lengths_hold_their_edges(case, H):
    cls = dc.classes(case, H)
    calls = dc.calls(case, H)
    ota = dc.LANES[case]
    full, mid = (4096, 2002) if case == "short_taps" else (32768, 20002)
    assert [c.G for c in calls] == [1, 1, 1, 3, 1, 1, 1] and calls[5].S == 0
    for c, want in zip(calls, (full, 5001, 3, 4099, full, 0, mid)):
        assert abs(c.S - want) <= 3 and (c.S == want or any(want % k.D == 0 for k in cls)), (c, want)
        assert c.S == 0 or all(c.S % k.D for k in cls), c  # no length is a multiple of a decimation
    walked = dc.walk(case, H)
    tall = [k for k in cls if k.count >= 8]
    # every full call: at least three x-tiles per tall class, the last one partial
    for i in (0, 4):
        c, consumed = walked[i]
        assert abs(c.S - calls[0].S) <= 3 and (c.S == dc.max_input(case, H) or case == "short_taps")
        for k in tall:
            K = dc.grid_outputs(consumed, k.D, c.S * c.G)
            assert -(-K // ota) >= 3 and K % ota != 0, (case, H, i, k, K)
    # call 3: most classes without output
    c, consumed = walked[2]
    Ks = [dc.grid_outputs(consumed, k.D, c.S) for k in cls]
    if case in ("even", "all_even"):
        assert any(K == 0 for K in Ks) and any(K > 0 for K in Ks), Ks
    assert sum(K == 0 for K in Ks) >= (len(Ks) + 1) // 2 or case == "short_taps", Ks
    # the grouped call: for every class a block end strictly inside a 16-output phase entry -- in the full walk and in the shorter
    # sequences of test_flat_priority_loop and test_role_inside_the_tall_launch, which reach it from another stream position
    sequences = [dc.ALL_CALLS] + ([dc.FLAT_CALLS] if case in dc.FLAT_CASES else []) + ([dc.ROLE_CALLS] if case == dc.ROLE_CASE else [])
    for which in sequences:
        c, consumed = dc.walk(case, H, which)[which.index(3)]
        assert c.G == dc.GROUP_BLOCKS
        for k in cls:
            assert c.S >= k.D, (c, k)  # (every block of a grouped call holds an output: xl_bnd_next)
            j0 = dc.grid_j0(consumed, k.D)
            ends = [dc.grid_mstart(j0, k.D, c.S, g) for g in (1, 2)]
            assert any(e % dc.XL_PH_STRIDE for e in ends), (case, H, which, k, ends)
    # call 1 runs a tall class inside its zero history: it has outputs there whose windows reach below the join point (T - 1 > 0
    # samples that zero_below masks), and a later full call (5) finds the same class mature
    c, consumed = walked[0]
    assert consumed == 0 and any(k.T > 1 and dc.grid_outputs(0, k.D, c.S) > 0 for k in tall)
    assert all(walked[4][1] >= k.T - 1 for k in cls)


@pytest.mark.parametrize("H", [9, 12])
def test_mid_stream_join_is_a_class_of_its_own(probe, H):
    """test_tall_class_joins_mid_stream: H + 2 clients of (42, 505) that join behind call 2 have another grid than the old class (the
    old clients' consumed mod 42 is not 0) and no history: a group of their own in the tall launch, with zero_below masking (hv0 = 0),
    and, one call later, still short of their T - 1 samples"""
    walked = dc.walk("even", H)
    consumed = walked[2][1]
    assert consumed % 42 != 0
    cls = dc.classes("even", H)
    pop = [(c.D, c.T, c.count, consumed) for c in cls] + [(42, 505, H + 2, 0)]
    tall = {L["ct"]: L for L in probe(H, dc.max_input("even", H), dc.GROUP_BLOCKS, pop)}[H]
    assert [(g["D"], g["rem0"], g["hv0"], g["tiles"]) for g in tall["g"]] == [
        (42, consumed % 42, dc.XL_HCAP, [H] * 4), (42, consumed % 42, dc.XL_HCAP, [H, 3]), (42, 0, 0, [H, 2])], tall
    assert dc.describe_direct([(c.D, c.T, c.count) for c in cls] + [(42, 505, H + 2)], H).startswith(" h%d x 3 groups" % H)
    after3 = walked[2][0].S
    assert 0 < after3 < 504 and after3 % 42 != 0  # the next plan's record of the joiners: rem0 != 0, valid history below T - 1
    assert after3 + walked[3][0].S * walked[3][0].G >= 504  # they mature during the grouped call


@pytest.mark.parametrize("case,H", [(case, H) for case in dc.SPARSE_CASES for H in dc.HEIGHTS], ids=lambda v: str(v))
def test_sparse_block_has_single_term_windows(case, H):
    """No window of any client holds two non-zero samples; and for every fc = 0 client the oracle's float32 sums are its float64 sums
    rounded: each sum has a single non-zero term."""
    fmt, x = dc.sparse_input(case, H)
    n = dc.max_input(case, H)
    assert x.size == 2 * n and fmt != "cu8"
    nz = np.nonzero((x[0::2] != 0) | (x[1::2] != 0))[0]
    assert len(nz) >= 8 and np.all(x[2 * nz] != 0) and np.all(x[2 * nz + 1] != 0)  # impulses of both a real and an imaginary part
    assert np.diff(nz).min() > max(c.T for c in dc.classes(case, H))
    mags = np.abs(x[np.nonzero(x)].astype(np.float64))
    assert np.all(np.log2(mags) == np.round(np.log2(mags))) and len(set(mags)) >= 6  # powers of two
    assert len({int(p) % c.D for p in nz for c in dc.classes(case, H)[:1]}) >= min(dc.classes(case, H)[0].D, 3)
    seen = 0
    for k, D, taps, fc in dc.clients(case, H, tall_fc0=True):
        if fc != 0:
            continue
        a, b = dc.make_oracle(D, taps, 0, 2 * n), dc.make_oracle(D, taps, 0, 2 * n, sum_mode=1)
        ya, yb = a.process(fmt, x), b.process(fmt, x)
        assert len(ya) > 0 and np.count_nonzero(ya) > 0 and np.array_equal(ya, yb), (case, H, k)
        assert a.phase == (np.float32(1), np.float32(0))
        a.close()
        b.close()
        seen += 1
    assert seen == sum(c.count for c in dc.classes(case, H) if c.count >= 8)


@pytest.mark.parametrize("D,T", [(4, 1), (5, 3), (7, 7)])
def test_gap_oracle_is_the_oracle_where_the_oracle_is_defined(D, T):
    """On blocks that are multiples of D the reference's history count never underflows: GapOracle (T - 1 < D) must then hand the
    plain oracle's outputs and phases on unchanged, call by call -- and on ragged blocks of the same stream it must give the same
    outputs in all, each in the call that holds its newest sample."""
    from pyoracle import Oracle
    taps = dc.taps_of(T, 1, 5, D)
    x = dc.call_input("cs16", 977, 40 * D + 3 * D)
    plain, gap, ragged = Oracle(D, taps, 123456, dc.FS, 2 * 50 * D), dc.GapOracle(D, taps, 123456, dc.FS, 2 * 50 * D), \
        dc.GapOracle(D, taps, 123456, dc.FS, 2 * 50 * D)
    pos, outs = 0, []
    for n in (3 * D, 0, D, 17 * D, 2 * D, 20 * D):
        xb = x[2 * pos:2 * (pos + n)]
        ya, yb = plain.process("cs16", xb), gap.process("cs16", xb)
        assert np.array_equal(ya.view(np.uint32), yb.view(np.uint32)) and len(ya) == n // D, (D, T, n)
        assert [v.tobytes() for v in plain.phase] == [v.tobytes() for v in gap.phase] and gap.skip == 0
        outs.append(ya)
        pos += n
    whole, pos, count = np.concatenate(outs), 0, 0
    for n in (D + 1, 1, 2 * D - 1, 3, 0, 11 * D + 2, 29 * D - 6):
        y = ragged.process("cs16", x[2 * pos:2 * (pos + n)])
        first = -(-pos // D)
        assert len(y) == -(-(pos + n) // D) - first, (D, T, pos, n, len(y))  # the outputs whose newest sample k D lies in the block
        if T == 1:  # one tap: no rounding beside the phase's, whose renormalisation points differ between the two block sequences
            assert np.allclose(y, whole[first:first + len(y)], rtol=1e-5, atol=0)
        count += len(y)
        pos += n
    assert pos == 43 * D and count == len(whole)
    for o in (plain, gap, ragged):
        o.close()
