"""Host side of the candidate tests (tests/test_gpu_conv_pick.py): every shape of the case tables
in tests/conv_pick.py reaches the timed choice it is listed under -- and every boundary shape
misses it -- by the library's own predicates (the C ABI answers them without a device); the
tags of the tables are exactly the `_pick_any` sites of op/conv.py; and the forcing helper
fails a test that consults a site it did not name."""
import ast
import os

import pytest

import conv_pick as cp
from conftest import PKG


@pytest.mark.parametrize("case", cp.F3_CASES, ids=cp.case_id)
def test_f3_shapes_reach_the_choice(case):
    N, cin, cout, H, W = case
    assert cp.reaches_f3(*case)
    assert cp.wino_fwd_form(*case) == ("pair" if case == cp.F3_PAIR_FORM else "wino")
    if case == cp.F3_CASES[1]:  # what the table says of it
        assert cin % 16 != 0 and cout % 64 != 0 and N % 2 == 1


@pytest.mark.parametrize("case", cp.D3_CASES, ids=cp.case_id)
def test_d3_shapes_reach_the_choice(case):
    N, c0, c1, H, W = case
    assert c0 != c1, "asymmetric channels: exchanging them must not cancel"
    assert cp.reaches_d3(*case)
    assert cp.wino_fwd_form(*case) == ("pair" if case == cp.D3_PAIR_FORM else "wino")


@pytest.mark.parametrize("case", cp.W3_CASES, ids=cp.case_id)
def test_w3_shapes_reach_the_choice(case):
    assert cp.reaches_w3(*case)


def test_w3_large_image_is_reached_through_the_cout_alone():
    from op import conv
    N, cin, cout, H, W = cp.W3_CASES[3]
    assert H * W > conv._SMALL_IMG_MAX_HW and cout % 64 != 0 and cp.reaches_w3(N, cin, cout, H, W)


@pytest.mark.parametrize("case", cp.WSC_CASES, ids=cp.case_id)
def test_wsc_shapes_reach_the_choice(case):
    assert cp.reaches_wsc(*case)


@pytest.mark.parametrize("case", cp.DSC_CASES, ids=cp.case_id)
def test_dsc_shapes_reach_the_choice(case):
    assert cp.reaches_dsc(*case)


@pytest.mark.parametrize("case", cp.W2_CASES, ids=[c[0] for c in cp.W2_CASES])
def test_w2_shapes_reach_the_choice_with_the_launch_they_name(case):
    from op.conv import lib
    name, kind, how, N1, N2, cin, cout, H, W, k, s, p = case
    assert N1 != N2 or name == "gen_k3s2", "unequal sources, so a swapped or repeated one shows"
    assert cp.w2_launch(kind, N1, N2, cin, cout, H, W, k, s, p) == how
    # the choice the separate launches reach in turn (forced too by the test)
    nested = cp.W2_NESTED[name]
    for n in (N1, N2):
        if kind[0] == "3x3":
            assert cp.reaches_w3(n, cin, cout, H, W) == (nested == "w3")
            assert (not cp.reaches_w3(n, cin, cout, H, W)
                    and cp.reaches_wsc(n, cin, cout, H, W, 3)) == (nested == "wsc")
        elif kind[0] == "gen":
            assert nested is None and not (k in (1, 3) and s == 1 and cout <= 4)
        else:
            both = bool(lib.bpk_gemm_nchw_wgrad_supported(n, cout, cin, H * W))
            assert both == (1 in cp.W2_CANDIDATES.get(name, (0, 1))), \
                "the 1x1 GEMM weight gradient (candidate 1) takes multiples of 16 only"


def test_boundary_shapes_consult_nothing():
    from op import conv
    N, cin, cout, H, W = cp.F3_BOUNDARY
    assert cp.wino_fwd_form(*cp.F3_BOUNDARY) == "wino" and H * W > conv._SMALL_IMG_MAX_HW
    assert not cp.reaches_f3(*cp.F3_BOUNDARY)
    assert cp.wino_fwd_form(*cp.D3_BOUNDARY) == "wino" and not cp.reaches_d3(*cp.D3_BOUNDARY)
    N, cin, cout, H, W = cp.W3_BOUNDARY
    assert conv.lib.bpk_conv3x3_wino_wgrad_supported(N, cin, cout, H, W)
    assert not cp.reaches_w3(*cp.W3_BOUNDARY)
    assert not cp.reaches_wsc(*cp.WSC_BOUNDARY) and not cp.reaches_dsc(*cp.DSC_BOUNDARY)
    # H * W exactly at the limit is inside
    assert cp.F3_CASES[2][3] * cp.F3_CASES[2][4] == conv._SMALL_IMG_MAX_HW


def test_second_order_and_groupnorm_cases_reach_their_sites():
    N, cin, cout, H, W = cp.SECOND_ORDER_CASE
    assert cp.reaches_f3(N, cin, cout, H, W)          # the forward, and conv(x, ggw)
    assert cp.reaches_d3(N, cout, cin, H, W)          # backward-data: x has cout channels
    assert cp.reaches_w3(N, cin, cout, H, W)          # the weight gradient
    N, cin, cout, H, W = cp.GN_CASE
    assert cin % cp.GN_GROUPS == 0
    assert cp.wino_fwd_form(N, cin, cout, H, W) == "wino"
    assert cp.reaches_d3(N, cout, cin, H, W) and cp.reaches_w3(N, cin, cout, H, W)


def _pick_any_tags():
    """The first element of the key of every `_pick_any(key, ...)` call in op/conv.py: the key
    is a tuple literal, or a name assigned one in the same function."""
    path = os.path.join(PKG, "op", "conv.py")
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    tags = []
    for fn in ast.walk(tree):
        if not isinstance(fn, ast.FunctionDef):
            continue
        for node in ast.walk(fn):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name)
                    and node.func.id == "_pick_any"):
                continue
            key = node.args[0]
            if isinstance(key, ast.Name):
                lits = [a.value for a in ast.walk(fn) if isinstance(a, ast.Assign)
                        and any(isinstance(t, ast.Name) and t.id == key.id for t in a.targets)]
                assert len(lits) == 1, f"line {node.lineno}: key `{key.id}` assigned {len(lits)} times"
                key = lits[0]
            assert isinstance(key, ast.Tuple) and isinstance(key.elts[0], ast.Constant) \
                and isinstance(key.elts[0].value, str), f"line {node.lineno}: key is no tagged tuple"
            tags.append((node.lineno, key.elts[0].value))
    return sorted(set(tags))


def test_every_pick_any_site_has_cases():
    """A seventh timed choice added to op/conv.py fails here until conv_pick.TAGS names it
    (and tests/test_gpu_conv_pick.py runs both of its candidates)."""
    tags = [t for _, t in _pick_any_tags()]
    assert len(tags) == len(set(tags)), f"a tag used by two sites: {tags}"
    assert set(tags) == set(cp.TAGS) and len(cp.TAGS) == len(set(cp.TAGS)), tags


def test_forced_fails_on_an_unnamed_site_and_checks_the_index(monkeypatch):
    from op import conv
    log = cp.forced(monkeypatch, {"f3": 1, "w3": 5})

    def never():
        raise AssertionError("a forced choice ran a timer")
    key = ("f3", (1, 8, 8, 16), (16, 8, 3, 3), False, False)
    assert conv._pick_any(key, [lambda: "a", lambda: "b"]) == "b"
    assert conv._decide(key, [never, never]) == 1
    assert cp.reached(log, "f3") == [key, key] and cp.reached(log, "d3") == []
    with pytest.raises(AssertionError, match="not forced"):
        conv._decide(("d3", (1, 8, 8, 16)), [never, never])
    with pytest.raises(AssertionError, match="candidate 5 of 2"):
        conv._decide(("w3", (1, 8, 8, 16)), [never, never])
    log.append((("f3", "one candidate"), 1))
    with pytest.raises(AssertionError, match="1 candidates"):
        cp.reached(log, "f3")


def test_first_only_empties_every_cache(monkeypatch):
    from op import conv
    monkeypatch.setattr(conv, "_CHOICE", {("f3", 1): 1})
    monkeypatch.setattr(conv, "_TABLE", {conv._key_str(("f3", 2)): 1})
    cp.first_only(monkeypatch)

    def never():
        raise AssertionError("timed")
    assert conv._decide(("f3", 1), [never, never]) == 0
    assert conv._decide(("f3", 2), [never, never]) == 0
