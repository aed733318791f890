"""The inputs and expected values of the concurrency scenarios 8 to 16 (tests/concurrency_cases.py) without a GPU: every
builder gives the same case when called again, the references refuse every planted failure of scenarios 12 and 16 at the index
the scenario expects and accept every other call, the two sort columns of scenario 9 run different numbers of passes, the
opening of scenario 8 has terms of equal length on both sides of a group of five, the multiplicity calls of scenario 14 have
the sizes and the pass counts the scenario is about, and those of scenario 15 share their inputs."""
import time

import pytest

import concurrency_cases as cc
import logup_ref
import lookup_ref
import open_ref
import perm_ref

P, RI = cc.P, cc.RI
BUILDERS = {"8": cc.scenario8, "9": cc.scenario9, "10": lambda: {str(k): cc.scenario10(k) for k in range(4)}, "11": lambda: {"shared": cc.scenario11()},
            "12": cc.scenario12, "13": cc.scenario13, "14": cc.scenario14, "15": cc.scenario15, "16": cc.scenario16}


def _specs(case):
    return [sp for name in sorted(case) if name != "options" for sp in case[name]]


@pytest.fixture(scope="module")
def built():
    t0 = time.perf_counter()
    made = {name: fn() for name, fn in BUILDERS.items()}
    made["seconds"] = time.perf_counter() - t0
    return made


def test_builders_are_deterministic_and_quick(built):
    print("scenarios 8-16 built in %.2f s" % built["seconds"])
    assert built["seconds"] < 30                                            # (measured: profiles/concurrency/NOTES.md)
    for name, fn in BUILDERS.items():
        again = _specs(fn())
        assert [sp.fingerprint() for sp in again] == [sp.fingerprint() for sp in _specs(built[name])], name
    prints = [sp.fingerprint() for name in BUILDERS if name != "9" for sp in _specs(built[name])]
    assert len(set(prints)) == len(prints)                                  # no two calls alike ...
    assert len({sp.fingerprint() for sp in _specs(built["9"])}) == 5       # ... but in scenario 9: two transforms, one combination, two sorts
    assert len({sp.fingerprint() for k in range(4) for sp in built["10"][str(k)]}) == 4 * 7        # every context of scenario 10 has inputs of its own


def test_every_call_fits_its_buffers(built):
    for name in BUILDERS:
        for sp in _specs(built[name]):
            for out, cap, want, init in sp.outs:
                assert len(want) % 32 == 0 and len(want) <= cap * 32, (name, sp, out)
                assert init is None or init.nbytes <= cap * 32
                assert not sp.error or want == (b"" if init is None else init.tobytes()), (name, sp, out)   # a refused call leaves its output as it was
            assert sp.error or sp.index is None
            assert not (sp.error and sp.small)


def _ints_of(sp, name):
    return cc._ints(sp.ins[name])


def test_planted_failures_of_scenario_12(built):
    a, b = built["12"]["A"], built["12"]["B"]
    assert not any(sp.error for sp in b) and sorted(sp.op for sp in b) == ["fft", "fp", "pair", "quotient"]
    assert [sp.error for sp in a] == [False, True, False, True, False, True, False, True, False, True, False]
    bad = {sp.op: sp for sp in a if sp.error}
    assert sorted(bad) == ["divide", "fft", "fp", "lincomb", "pair"]
    for k in range(1, len(a), 2):                                           # every refusal is followed by the good call of the same entry
        assert a[k].op == a[k + 1].op and not a[k + 1].error
    # lookup_permute: the lowest row of the smallest missing value, which is not the lowest row that misses
    sp = bad["pair"]
    A, S = [v * RI % P for v in _ints_of(sp, "A")], [v * RI % P for v in _ints_of(sp, "S")]
    missing = [r for r, v in enumerate(A) if v not in set(S)]
    assert missing == [40, 2222] and A[2222] < A[40]
    with pytest.raises(lookup_ref.NotInTable) as e:
        lookup_ref.permute_expression_pair(A, S)
    assert e.value.index == sp.index == lookup_ref.missing_row(A, S) == 2222 and sp.status == cc.NOT_IN_TABLE
    # fraction_products: zero denominators at rows 1234 (two columns) and 4711
    sp = bad["fp"]
    nums = [[v * RI % P for v in _ints_of(sp, "num%d" % k)] for k in range(sp.args["n_num"])]
    dens = [[v * RI % P for v in _ints_of(sp, "den%d" % k)] for k in range(sp.args["n_den"])]
    assert [r for r in range(sp.args["n"]) if any(c[r] == 0 for c in dens)] == [1234, 4711]
    with pytest.raises(perm_ref.ZeroDenominator) as e:
        perm_ref.fraction_products(nums, dens, sp.args["n"], 1, sp.args["tap"])
    assert e.value.index == sp.index == 1234 and sp.status == cc.DIV_ZERO
    # divide_by_roots: 2 coefficients, 4 roots: stage 2 meets the empty polynomial
    sp = bad["divide"]
    with pytest.raises(OverflowError) as e:
        open_ref.divide_roots(_ints_of(sp, "a"), [v * RI % P for v in cc._ints(sp.args["roots"])], P)
    assert e.value.args[0] == sp.index == sp.args["length"] == 2 < sp.args["roots"].shape[0] and sp.status == cc.OVERFLOW
    # fft: omega is no primitive 2^logn-th root
    sp = bad["fft"]
    w, logn = cc._ints(sp.args["omega"])[0] * RI % P, sp.args["logn"]
    assert pow(w, 1 << logn, P) == 1 and pow(w, 1 << (logn - 1), P) != P - 1 and sp.status == cc.BAD_ARG and sp.index is None
    good = a[a.index(sp) + 1]
    w = cc._ints(good.args["omega"])[0] * RI % P
    assert good.args["logn"] == logn and pow(w, 1 << (logn - 1), P) == P - 1 and good.outs[0][3].tobytes() == sp.outs[0][3].tobytes()
    assert a[0].op == "fft" and a[0].args["logn"] != logn                  # the table the context holds before is another size's
    # poly_lincomb: a capacity one element below the combination's length
    sp = bad["lincomb"]
    good = a[a.index(sp) + 1]
    assert sp.outs[0][1] == max(sp.args["lens"]) - 1 == good.outs[0][1] - 1 and sp.status == cc.BAD_ARG and len(good.outs[0][2]) == 32 * good.outs[0][1]


def test_good_calls_are_accepted(built):
    """every call that is not a planted failure: the reference gave a full result"""
    for name in BUILDERS:
        for sp in _specs(built[name]):
            if not sp.error:
                assert sp.status == cc.OK and all(len(want) for _, _, want, _ in sp.outs), (name, sp)
    sp = [s for s in built["12"]["A"] if s.op == "pair" and not s.error][0]
    A, S = [v * RI % P for v in _ints_of(sp, "A")], [v * RI % P for v in _ints_of(sp, "S")]
    assert lookup_ref.missing_row(A, S) is None
    assert cc._mont(lookup_ref.permute_closed_form(A, S)[1]).tobytes() == sp.outs[1][2]              # (the closed form against the pop loop)


def test_sort_columns_of_scenario_9(built):
    case = built["9"]
    (ka, sa), = [(k, sp) for k, sp in enumerate(case["A"]) if sp.op == "sort"]
    (kb, sb), = [(k, sp) for k, sp in enumerate(case["B"]) if sp.op == "sort"]
    assert ka == kb and sa.args["n"] == sb.args["n"]
    pa = lookup_ref.live_passes([v * RI % P for v in _ints_of(sa, "keys")])
    pb = lookup_ref.live_passes([v * RI % P for v in _ints_of(sb, "keys")])
    assert pa == list(range(8)) and len(pb) == lookup_ref.MAX_PASSES        # upper limbs shared: 24 passes skipped; random keys: none
    assert lookup_ref.sort_bytes(sa.args["n"], len(pa)) != lookup_ref.sort_bytes(sb.args["n"], len(pb))
    # the transforms: where one context alternates two sizes the other repeats one, and halfway they change places
    logn = {name: [sp.args["logn"] if sp.op == "fft" else None for sp in case[name]] for name in "AB"}
    assert logn["A"] == [11, 12, 11, 12, None, None, 12, 12, 12, 12] and logn["B"] == [12, 12, 12, 12, None, None, 11, 12, 11, 12]
    assert case["A"][4] is case["B"][4] and case["A"][4].op == "lincomb" and case["options"] == {"A": {"open_group": 1}, "B": {}}


def test_open_case_of_scenario_8(built):
    (sp,) = [s for s in built["8"]["B"] if s.op == "quotient"]
    lens = sp.args["lens"]
    assert len(lens) == 7 and max(lens) == 16385 and len(set(lens)) >= 4 and sp.args["low"].shape[0] == 3 and sp.args["roots"].shape[0] == 3
    groups = cc.term_groups(lens)
    assert [len(g) for g in groups] == [5, 2]
    assert groups[0][-1] == groups[1][0] and len(set(groups[0])) >= 2 and len(set(groups[1])) >= 2 and cc.straddles(lens)
    assert not cc.straddles([9, 9, 9, 9, 9, 4, 4]) and not cc.straddles([7, 7, 7, 7, 7, 7])
    # the sizes the issue names for the single-block stages
    a = {s.op + str(k): s for k, s in enumerate(built["8"]["A"])}
    assert [int(n) for _, n in a["kate5"].args["rows"]] == [16385] and (a["mul6"].args["la"], a["mul6"].args["lb"]) == (300, 257)
    assert (a["mul7"].args["la"], a["mul7"].args["lb"]) == (31, 40) and a["fft0"].args["logn"] == 12
    b = {s.op: s for s in built["8"]["B"]}
    assert b["fp"].args["n"] == 8193 and b["sort"].args["n"] == 5000 and b["pair"].args["n"] == 4096 and b["fsums"].args["n"] == 4097


def _mult_columns(sp):
    """(the columns the call takes, the table) of a multiplicity Spec, standard form"""
    cols = [[v * RI % P for v in _ints_of(sp, name)] if name else [] for name in sp.args["cols"]]
    return cols, [v * RI % P for v in _ints_of(sp, "T")]


def test_multiplicity_calls_of_scenario_14(built):
    a, b = built["14"]["A"], built["14"]["B"]
    assert [sp.op for sp in a] == ["mult", "pair", "sort"] and [sp.op for sp in b] == ["mult", "quotient", "mult"]
    assert not any(sp.error for sp in a + b)
    ma, mb, small = a[0], b[0], b[2]
    assert ma.args["lens"] == mb.args["lens"] and len(ma.args["lens"]) == 3 and sum(ma.args["lens"]) == 4099 and len(set(ma.args["lens"])) == 3
    assert ma.args["t"] == mb.args["t"] == 1025 and (ma.args["form"], mb.args["form"]) == (cc.MONT, cc.CANON)
    assert sorted(ma.ins) == sorted(mb.ins) and all(ma.ins[k].tobytes() == mb.ins[k].tobytes() for k in ma.ins)      # the same inputs
    cols, table = _mult_columns(ma)
    assert len(set(table)) < len(table) and [len(c) for c in cols] == ma.args["lens"]                              # duplicates in the table
    m = logup_ref.multiplicities(cols, table)
    assert sum(m) == 4099 and cc._mont(m).tobytes() == ma.outs[0][2] and cc._arr(m).tobytes() == mb.outs[0][2] != ma.outs[0][2]
    assert ma.args["passes"] == (logup_ref.MAX_PASSES, logup_ref.MAX_PASSES)                                        # full-width keys: no pass skipped
    cols, table = _mult_columns(small)
    assert max(table) < 1 << 16 and small.args["passes"] == (2, 2) and None in small.args["cols"]                  # keys below 2^16, a NULL column
    assert list(small.small[0]) == [4, 2 * logup_ref.MAX_PASSES - 4] and list(ma.small[0]) == [2 * logup_ref.MAX_PASSES, 0]
    assert list(a[2].small[0]) == [8, logup_ref.MAX_PASSES - 8]                                                     # A's sort: upper limbs shared


def test_shared_inputs_of_scenario_15(built):
    specs = built["15"]["0"] + built["15"]["1"]
    first = specs[0]
    assert sorted(first.ins) == ["T", "c0", "c1", "c3", "c4", "c5"]                                                 # (column 2 has no rows)
    subsets = []
    for sp in specs:
        assert sorted(sp.ins) == sorted(first.ins) and all(sp.ins[k].tobytes() == first.ins[k].tobytes() for k in sp.ins)
        cols, table = _mult_columns(sp)
        m = logup_ref.multiplicities(cols, table)
        assert sum(m) == sum(sp.args["lens"]) and (cc._mont(m) if sp.args["form"] == cc.MONT else cc._arr(m)).tobytes() == sp.outs[0][2]
        subsets.append(tuple(sp.args["cols"]))
    assert len(set(subsets)) == 4 and any(None in s for s in subsets)                                               # different subsets, a NULL column among them
    assert {sp.args["form"] for sp in built["15"]["0"]} == {sp.args["form"] for sp in built["15"]["1"]} == {cc.MONT, cc.CANON}
    assert len({sp.outs[0][2] for sp in specs}) == 4


def test_planted_failures_of_scenario_16(built):
    a, b = built["16"]["A"], built["16"]["B"]
    assert not any(sp.error for sp in b) and all(sp.op == "mult" for sp in a + b) and len(b) == 3
    assert [sp.error for sp in a] == [False, True, False, True, False, True, False, True, False]
    one, later, k17, overlap = [sp for sp in a if sp.error]
    # one missing value
    cols, table = _mult_columns(one)
    assert [(c, r) for c, col in enumerate(cols) for r, v in enumerate(col) if v not in set(table)] == [(0, 123)]
    assert one.index == logup_ref.missing_position(cols, table) == 123 and one.status == cc.NOT_IN_TABLE
    # three missing values: the smallest one in column 2, behind a larger one in column 0 -- the position lies in a later column
    cols, table = _mult_columns(later)
    gone = [(c, r, v) for c, col in enumerate(cols) for r, v in enumerate(col) if v not in set(table)]
    assert [(c, r) for c, r, _ in gone] == [(0, 5), (2, 77), (3, 299)] and min(gone, key=lambda g: g[2])[:2] == (2, 77)
    lens = later.args["lens"]
    assert lens[1] == 0 and later.args["cols"][1] is None
    assert later.index == logup_ref.missing_position(cols, table) == lens[0] + lens[1] + 77 and later.status == cc.NOT_IN_TABLE
    with pytest.raises(logup_ref.NotInTable) as e:
        logup_ref.multiplicities(cols, table)
    assert e.value.index == later.index
    # k = 17: one column above the limit, every pointer and length legal
    assert len(k17.args["lens"]) == len(k17.args["cols"]) == logup_ref.MAX_COLS + 1 and k17.status == cc.BAD_ARG and k17.index is None
    assert all(n == 1 for n in k17.args["lens"]) and all(k17.ins[name].shape[0] >= 1 for name in k17.args["cols"])
    assert logup_ref.plan(k17.args["lens"], k17.args["t"]) is None and logup_ref.plan(k17.args["lens"][:16], k17.args["t"]) is not None
    # the output one element into the table: t elements from there end inside the table's buffer and its 4096-byte zone
    name, at = overlap.args["out_at"]
    assert name == "T" and 0 < at and 32 * at <= 4096 and overlap.ins["T"].shape[0] == overlap.args["t"] and overlap.status == cc.BAD_ARG
    for k in range(1, len(a), 2):                                           # the good call behind every refusal
        good = a[k + 1]
        cols, table = _mult_columns(good)
        assert not good.error and logup_ref.missing_position(cols, table) is None and len(good.outs[0][2]) == 32 * good.args["t"]
        assert good.args["lens"] == a[0].args["lens"] and a[k].outs[0][2] == b""


# ---- scenarios 17 to 20: the transform over G1 and the inner-product argument ---------------------------------------------------
IPA_BUILDERS = {"18": lambda: {"shared": cc.scenario18()}, "19": cc.scenario19, "20": lambda: {str(k): cc.scenario20(k) for k in range(4)}}


@pytest.fixture(scope="module")
def built_ipa():
    return {name: fn() for name, fn in IPA_BUILDERS.items()}


def test_ipa_builders_are_deterministic_and_fit_their_buffers(built_ipa):
    for name, fn in IPA_BUILDERS.items():
        assert [sp.fingerprint() for sp in _specs(fn())] == [sp.fingerprint() for sp in _specs(built_ipa[name])], name   # reproducible from the seed
        for sp in _specs(built_ipa[name]):
            for out, cap, want, init in sp.outs:
                assert len(want) % 32 == 0 and len(want) <= cap * 32, (name, sp, out)
                assert not sp.error or want == (b"" if init is None else init.tobytes()), (name, sp, out)   # a refused call leaves its output as it was
            assert not (sp.error and sp.small)
    prints = [sp.fingerprint() for name in IPA_BUILDERS for sp in _specs(built_ipa[name])]
    assert len(set(prints)) == len(prints)
    assert len({sp.fingerprint() for k in range(4) for sp in built_ipa["20"][str(k)]}) == 4 * 5          # every context of scenario 20 has inputs of its own
    assert [sp.op for sp in built_ipa["20"]["0"]] == ["ecfft", "round", "fold", "uround", "fft"]
    assert [(sp.args.get("logn"), sp.args.get("half"), sp.args.get("q")) for sp in built_ipa["20"]["0"]] == [(7, None, None), (None, 257, None), (None, 65, None), (None, 64, 2), (10, None, None)]


def test_opening_of_scenario_17_is_the_references():
    one, two = cc.scenario17(), cc.scenario17()
    assert all(one["want"][k].tobytes() == two["want"][k].tobytes() for k in one["want"]) and one["ecfft"].fingerprint() == two["ecfft"].fingerprint()
    assert one["k"] == 10 and one["p"].shape == (1024, 4) and one["g"].shape == (1024, 8) and 0 < one["fold_rounds"] < 10
    assert one["options"] == {"A": {}, "B": {"field": 1, "window_bits": 13}} and one["ecfft"].args["logn"] == 8
    want = one["want"]
    us = [v * RI % P for v in cc._ints(want["u"])]
    assert len(set(us)) == 10 and all(0 < u < P for u in us)
    # the reference's own closing identities on this opening: c b'[0] = <p, b> + sum (u^-1 value_l + u value_r), b'[0] = <s, b>
    p = [v * RI % P for v in cc._ints(one["p"])]
    b = cc.ipa_ref.powers(cc._ints(one["x"])[0] * RI % P, 1024)
    c, b_fin = (cc._ints(want[k])[0] * RI % P for k in ("c", "b"))
    vls, vrs = ([v * RI % P for v in cc._ints(want[k])] for k in ("value_l", "value_r"))
    assert c * b_fin % P == cc.ipa_ref.opening_values(p, b, vls, vrs, us)
    assert b_fin == cc.ipa_ref.inner(cc.ipa_ref.compute_s(us, 1), b)
    # every challenge is the hash of its round's L and R
    assert all(cc.opening_challenge(want["L"][j], want["R"][j]) == us[j] for j in range(10))


def test_shared_buffers_of_scenario_18_are_read_only(built_ipa):
    specs = built_ipa["18"]["shared"]
    assert [sp.op for sp in specs] == ["round", "uround", "final", "ecfft", "ecfft"] and not any(sp.error for sp in specs)
    whole = {"p": specs[0].ins["p"], "b": specs[0].ins["b"], "G": specs[0].ins["g"]}
    assert whole["G"].shape == (cc.SHARED_ROWS, 8) and whole["p"].shape == (cc.SHARED_ROWS, 4)
    for sp in specs:
        assert sp.ins and all(name in ("p", "b", "g", "G") for name in sp.ins)
        for name, arr in sp.ins.items():                                    # a prefix of the shared vector, never an output
            assert arr.tobytes() == whole["G" if name == "g" else name][:arr.shape[0]].tobytes(), (sp, name)
        assert all(out == "out" and init is None for out, _, _, init in sp.outs)     # outputs of the call's own, none in place
    assert specs[3].args["lagrange"] is False and specs[4].args["lagrange"] is True and specs[4].args["rows"] == cc.SHARED_ROWS


def test_planted_refusals_of_scenario_19(built_ipa):
    a, b = built_ipa["19"]["A"], built_ipa["19"]["B"]
    assert built_ipa["19"]["options"] == {"A": {"validate_points": 1}, "B": {}}
    assert not any(sp.error for sp in b) and sorted(sp.op for sp in b) == ["ecfft", "final", "fold", "round", "uround"]
    assert [sp.error for sp in a] == [False, True, False, True, False, True, False, True, False, True, False]
    for k in range(1, len(a), 2):                                           # every refusal is followed by the good call of the same entry
        assert a[k].op == a[k + 1].op and not a[k + 1].error and a[k].status == cc.BAD_ARG
    off, inverse, zero, omega, overlap = (a[k] for k in range(1, len(a), 2))
    g = off.ins["g"]                                                        # one generator off the curve, its index reported
    bad_rows = [i for i in range(g.shape[0]) if g[i].any() and not cc.cref.is_on_curve(0, g[i])]
    assert bad_rows == [off.index] and all(sp.index is None for sp in (inverse, zero, omega, overlap))
    u, ui = (cc._ints(inverse.args[k].reshape(1, 4))[0] * RI % P for k in ("u", "u_inv"))
    assert u * ui % P != 1 and 0 < u < P
    assert 0 in [v for v in cc._ints(zero.args["u"])] and zero.args["q"] == 2
    w = cc._ints(omega.args["omega"].reshape(1, 4))[0] * RI % P
    n = 1 << omega.args["logn"]
    assert pow(w, n, P) == P - 1                                            # a root of order 2n: no 2^logn-th root
    assert overlap.args["overlap"] and not any(sp.args.get("overlap") for sp in a if sp is not overlap and sp.op == "ecfft")
