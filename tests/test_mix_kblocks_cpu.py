"""CPU tests of tests/mix_kblock_cases.py: the table holds exactly the mix-kernel instantiations that the four dispatch switches of
xl_mixh.hip, xl_mixh2.hip and xl_mixf32.hip can reach -- the labels are parsed from the sources, not copied, so an instantiation added
later without a case fails here --, every case is a class the plan admits, and every call of the GPU test
(tests/test_mix_kblocks_gpu.py) takes the polyphase launches with two or more passes of which the last is partial."""
import os
import re

import pytest

import mix_kblock_cases as mk
import poly_edges as pe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdr-server_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define %s (\d+)u?\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _function_body(text, signature):
    """the text between the braces of the function whose definition holds `signature`"""
    at = text.index(signature)
    i = text.index("{", at)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
        j += 1


def _switch(text, signature):
    """The `switch (a.nkb)` of a launcher -> ({label: statement}, statement of `default:`)"""
    body = _function_body(text, signature)
    assert body.count("switch (") == 1 and "switch (a.nkb) {" in body, signature
    sw = _function_body(body, "switch (a.nkb)")
    cases = {}
    for m in re.finditer(r"^\s*case (\d+):(.*)$", sw, re.M):
        assert int(m.group(1)) not in cases
        cases[int(m.group(1))] = m.group(2).strip()
    default = re.findall(r"^\s*default:(.*)$", sw, re.M)
    assert len(default) == 1 and len(cases) + 1 == len([ln for ln in sw.splitlines() if ln.strip()]), sw  # (nothing else in it)
    return cases, default[0].strip()


def _template_arg(statement, callee):
    m = re.match(r"%s<(\d+)>\(a, grid, s\); break;" % callee, statement)
    assert m, statement
    return int(m.group(1))


@pytest.fixture(scope="module")
def reach():
    """{arm: the set of k-block counts whose instantiation (or, streamed, whose run-time count) a switch can reach}"""
    hdr, mixh, mixh2, mixf = _read("xl_polyphase.h"), _read("xl_mixh.hip"), _read("xl_mixh2.hip"), _read("xl_mixf32.hip")
    nkb_4w, nkb_max = _define(hdr, "XLP_NKB_4W"), _define(hdr, "XLP_NKB_MAX")
    # ---- the narrow two-half kernel: one label per count, three forms per label
    narrow, narrow_default = _switch(mixh, "hipError_t xlp_launch_mix(")
    for n, st in narrow.items():
        assert _template_arg(st, "xlp_launch_mix_mfma_n") == n
    assert narrow_default.startswith("xlp_mix_wide_launch(a, s); break;")
    forms = _function_body(mixh, "static void xlp_launch_mix_mfma_n(")
    assert re.findall(r"xlp_mix_mfma_kernel<NKB, ([a-z, ]+)>", forms) == ["true", "false, true", "false"], forms  # SEG, IMG, plain
    assert "static_assert(NKB <= (int)XLP_NKB_4W" in mixh and sorted(narrow) == list(range(1, nkb_4w + 1))
    # ---- the wide two-half kernel: labels, and the count the default stands for; xlp_launch_mix refuses more than XLP_NKB_MAX
    wide, wide_default = _switch(mixh2, "void xlp_mix_wide_launch(")
    for n, st in wide.items():
        assert _template_arg(st, "xlmh_launch_n") == n
    wide_counts = set(wide) | {_template_arg(wide_default, "xlmh_launch_n")}
    assert "a0.nkb > XLP_NKB_MAX" in _function_body(mixh, "hipError_t xlp_launch_mix(")
    assert "static_assert(NKB > (int)XLP_NKB_4W && NKB <= (int)XLP_NKB_MAX" in mixh2
    assert min(wide_counts) == nkb_4w + 1 and max(wide_counts) == nkb_max and not set(narrow) & wide_counts
    wide_forms = _function_body(mixh2, "static void xlmh_launch_n(")
    assert re.findall(r"xlp_mix_mfma_wide_kernel<NKB, ([a-z]+)>", wide_forms) == ["true", "false"], wide_forms  # SEG, plain
    # ---- the float32 kernel with resident operands, and the streamed one behind the default
    f32, f32_default = _switch(mixf, "hipError_t xlp_launch_mix_f32(")
    for n, st in f32.items():
        assert _template_arg(st, "xlmf_launch_n") == n
    assert "xlp_mix_f32_stream_kernel" in f32_default
    assert sorted(f32) == list(range(1, max(f32) + 1))
    # (the operand image: xlp_ximg_eligible admits up to XLP_NKB_4W, the narrow kernel's counts)
    assert "nkb <= XLP_NKB_4W" in _function_body(hdr, "static inline bool xlp_ximg_eligible(")
    return {"plain": set(narrow) | wide_counts, "seg": set(narrow) | wide_counts, "img": set(narrow), "f32": set(f32),
            "stream": {max(f32) + 1}}  # (the first streamed class)


def test_table_holds_every_reachable_instantiation(reach):
    assert set(reach) == set(mk.ARMS) == {c.arm for c in mk.CASES}
    for arm in mk.ARMS:
        got = {-(-c.D // 8) for c in mk.CASES if c.arm == arm}
        assert got == reach[arm], (arm, sorted(got), sorted(reach[arm]))
        assert {c.nkb for c in mk.CASES if c.arm == arm} == got
    assert sorted(mk.tests()) == sorted((arm, n) for arm in mk.ARMS for n in reach[arm])


def test_two_decimations_per_count():
    """D_full = 8 nkb has no padding row, D_pad = 8 nkb - 7 seven (nkb = 1: D = 3, five); both give the same count; every (arm, nkb,
    format, transform length) of 37 clients runs both."""
    for arm, nkb in mk.tests():
        cases = [c for c in mk.cases_of(arm, nkb) if c.clients == mk.CLIENTS]
        d_pad, d_full = mk.decimations(nkb) if arm != "stream" else (113, 120)
        assert d_full % 8 == 0 and d_pad % 8 in (1, 3) and -(-d_pad // 8) == -(-d_full // 8) == d_full // 8 == nkb
        variants = {(c.fmt, c.M) for c in cases}
        assert {(c.fmt, c.M, c.D) for c in cases} == {(f, m, d) for f, m in variants for d in (d_pad, d_full)}, (arm, nkb)
        assert len(cases) == 2 * len(variants)


def test_arms_formats_and_transform_lengths():
    by = {}
    for c in mk.CASES:
        by.setdefault((c.arm, c.nkb), []).append(c)
        opts = dict(c.options)
        assert len(opts) == len(c.options) and opts["polyphase"] == 1 and opts["polyphase_m"] == c.M
        assert (opts.get("mix_kernel"), opts.get("mix_operand_image"), c.tag, c.not_tag) == {
            "plain": (1, 0, " mix=mfma", "/img"), "seg": (1, None, " mix=mfma", "/img"), "img": (1, 1, " mix=mfma/img", None),
            "f32": (3, None, " mix=mf32", None), "stream": (None, None, " mix=mf32", None)}[c.arm]
    for (arm, nkb), cases in by.items():
        fmts, ms = {c.fmt for c in cases}, {c.M for c in cases}
        if arm == "stream":
            assert (fmts, ms) == ({"cu8"}, {128})
            continue
        assert ms == ({128} if nkb <= 8 else ({64, 128} if nkb in (9, 12, 14) else {64})), (arm, nkb)
        assert fmts == {"plain": {"cu8", "cs16"} if nkb in (9, 12) else {"cu8"}, "seg": {"cf32"}, "img": {"cu8"},
                        "f32": {"cf32"} if nkb % 2 else {"cu8"}}[arm], (arm, nkb)
        big = [c for c in cases if c.clients != mk.CLIENTS]
        assert [(c.clients, c.fmt) for c in big] == ([(160, "cu8")] if arm == "plain" and nkb in (4, 10, 14) else []), (arm, nkb)
    # (160 clients: a second column group of 128, partial; 37: wave 0 full, wave 1 with five columns)
    assert mk.CLIENTS == 32 + 5 and 128 < mk.CLIENTS_TWO_GROUPS < 256


def test_every_case_is_a_class_the_plan_admits():
    """xl_poly_form_classes: 2 <= taps per branch <= M / 2, D <= 504; here between 2 and 8 (what a 64-point class is given)"""
    for c in mk.CASES:
        A = pe.taps_per_branch(c.T, c.D)
        assert c.T == 4 * c.D + 1 and A == 5 and 2 <= A <= 8 and A <= c.M // 2 and c.D <= 504, c


def test_every_call_takes_two_or_more_polyphase_passes_the_last_one_partial():
    """Blocks of 16384 samples.  An 8-block call gives its largest client (all members share one grid) at least 512 outputs -- the
    polyphase launches, not the direct fall-back -- in every case, and at least 17 segments wherever the arithmetic allows; the seven
    cases where it does not (128 points, more than 66 branches) take 16 blocks, and no other case does.  In all three calls of a case:
    17 or more segments, the last pass partial."""
    sixteen = set()
    for c in mk.CASES:
        V = pe.valid_points(c.M, c.T, c.D)
        assert V == c.M - 5 + 1
        assert pe.use_poly(pe.grid_outputs(0, c.D, mk.NSAMP, 8))
        nseg8 = pe.segments(pe.merge_points(c.D, mk.NSAMP, 8), V)
        assert c.blocks == (8 if nseg8 >= 17 else 16), c
        if c.blocks == 16:
            assert c.M == 128 and c.D > 66 and nseg8 < 17
            sixteen.add((c.D, c.M))
        consumed = 0
        for _ in range(3):
            assert pe.use_poly(pe.grid_outputs(consumed, c.D, mk.NSAMP, c.blocks))
            nseg = pe.segments(pe.merge_points(c.D, mk.NSAMP, c.blocks), V)
            assert nseg == mk.segments_of(c.D, c.T, c.M, c.blocks)
            assert nseg >= mk.MIN_SEGMENTS == pe.XLP_SEG + 1 and pe.passes(nseg) >= 2 and nseg % pe.XLP_SEG != 0, (c, nseg)
            assert nseg <= pe.nseg_cap(mk.NSAMP * c.blocks, c.D, V) - 1  # (inside the engine's segment capacity)
            consumed += mk.NSAMP * c.blocks
    assert sixteen == {(72, 128), (89, 128), (96, 128), (105, 128), (112, 128), (113, 128), (120, 128)}, sorted(sixteen)
