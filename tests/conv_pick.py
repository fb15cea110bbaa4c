"""Forcing the timed kernel choices of op/conv.py in tests, and the shapes that reach them.

op.conv decides some convolutions at run time: the first eager call of a distinct key times two
native candidates (`_pick_any` -> `_decide`) and keeps the faster.  A test that goes through
such a site therefore checks whichever candidate won on that machine at that moment.
`forced()` replaces `_decide` for one test, so the test names the candidate it runs, no timer
runs, and the test fails when a site it did not name is consulted or the site it names is not.

The case tables of tests/test_gpu_conv_pick.py live here, so tests/test_conv_pick_host.py can
show without a device, from the library's own predicates, that every shape reaches (or, for
the boundary shapes, misses) the site it is listed under.
"""
import math

TAGS = ("f3", "d3", "w3", "dsc", "wsc", "w2")


def forced(monkeypatch, picks):
    """Replace op.conv._decide: the candidate of a key tagged `t` is picks[t].  Returns the log
    [(key, number of candidates)] of every consultation.  A tag that `picks` does not name
    fails the test with the key; no candidate is ever timed."""
    from op import conv
    picks = dict(picks)
    log = []

    def decide(key, timers):
        log.append((key, len(timers)))
        if key[0] not in picks:
            raise AssertionError(f"conv choice not forced by this test: {key!r} "
                                 f"(forced: {sorted(picks)})")
        c = picks[key[0]]
        assert 0 <= c < len(timers), f"candidate {c} of {len(timers)} for {key!r}"
        return c
    monkeypatch.setattr(conv, "_decide", decide)
    return log


def reached(log, tag):
    """The keys consulted for `tag`, each of which must have offered two candidates."""
    keys = []
    for key, n in log:
        if key[0] == tag:
            assert n == 2, f"{key!r}: {n} candidates"
            keys.append(key)
    return keys


def case_id(case):
    return "-".join(str(v) for v in case)


def first_only(monkeypatch):
    """The setting of the op test modules: no timing and no inherited choice -- every site
    runs its first candidate (the kernel the tests' names and docstrings speak of)."""
    from op import conv
    monkeypatch.setattr(conv, "_PICK_FIRST", True)
    monkeypatch.setattr(conv, "_CHOICE", {})
    monkeypatch.setattr(conv, "_CHOICE_LOCAL", {})
    monkeypatch.setattr(conv, "_TABLE", {})


# ------------------------------------------------------------------------------- case tables
SQRT2 = math.sqrt(2.0)

# f3 (conv._fwd_impl): N, Cin, Cout, H, W
F3_CASES = [
    (1, 8, 16, 8, 16),      # one tile, one chunk
    (3, 24, 48, 16, 32),    # cin not a multiple of 16, cout padded to 64, odd batch
    (2, 64, 128, 32, 32),   # H * W exactly 1024
    (2, 16, 128, 40, 16),   # non-square
    (2, 32, 128, 8, 8),     # pair form
]
F3_PAIR_FORM = (2, 32, 128, 8, 8)
F3_VARIANTS = ("plain", "bias", "bias_skip")  # three keys per shape
F3_BOUNDARY = (1, 16, 16, 8, 144)             # H * W = 1152: Winograd, no choice

# d3 (conv._fwd_ft_impl(x, w)): N, w.shape[0] (= x's channels), w.shape[1] (= the result's), H, W
D3_CASES = [
    (3, 24, 32, 8, 16),
    (2, 128, 16, 16, 16),
    (2, 32, 128, 8, 8),     # pair form
]
D3_PAIR_FORM = (2, 32, 128, 8, 8)
D3_BOUNDARY = (1, 16, 16, 8, 144)

# w3 (conv._wgrad_impl): N, Cin, Cout, H, W
W3_CASES = [
    (1, 32, 16, 2, 16),     # minimal
    (3, 32, 48, 10, 48),    # small image
    (2, 32, 64, 8, 8),      # pair form
    (2, 64, 80, 64, 64),    # large image, reached only through Cout % 64
]
W3_BOUNDARY = (2, 32, 64, 64, 64)  # large image, Cout % 64 == 0: Winograd, no choice

# wsc (conv.conv2d_weight_select): N, Cin, Cout, H, W, K
WSC_CASES = [
    (2, 5, 1, 9, 13, 3),
    (2, 3, 3, 5, 7, 1),
    (1, 4, 2, 1, 1, 3),
]
WSC_BOUNDARY = (2, 5, 5, 9, 13, 3)  # Cout = 5: implicit GEMM, no choice

# dsc (conv.conv2d_input_select): N, Cin (<= 4, the gradient's channels), Cout, H, W
DSC_CASES = [
    (3, 1, 64, 16, 20),
    (3, 4, 64, 16, 20),
    (3, 2, 64, 16, 20),
    (3, 3, 64, 16, 20),
]
DSC_BOUNDARY = (3, 5, 64, 16, 20)  # Cin = 5: implicit GEMM, no choice

# w2 (conv._wgrad_pairs): name, kind, the two-source launch, N1, N2, Cin, Cout, H, W, k, stride, pad
GEN_S2P1 = ((2, 2), (1, 1), (1, 1), 1)  # cfg of conv2d_general: stride, padding, dilation, groups
W2_CASES = [
    ("wino", ("3x3",), "wino", 3, 5, 32, 16, 16, 16, 3, 1, 1),
    ("wino_pair", ("3x3",), "wino", 4, 6, 32, 48, 8, 8, 3, 1, 1),   # N1 even
    ("igemm3x3", ("3x3",), "igemm", 5, 3, 49, 32, 8, 8, 3, 1, 1),
    ("1x1_odd", ("1x1",), "igemm", 2, 3, 33, 17, 5, 5, 1, 1, 0),
    ("1x1", ("1x1",), "igemm", 2, 3, 48, 32, 4, 4, 1, 1, 0),
    ("gen_k4s2", ("gen", GEN_S2P1), "igemm", 2, 3, 6, 4, 9, 9, 4, 2, 1),
    ("gen_k3s2", ("gen", GEN_S2P1), "igemm", 4, 4, 16, 32, 12, 12, 3, 2, 1),
    ("small_cout", ("3x3",), "igemm", 2, 3, 5, 2, 6, 8, 3, 1, 1),   # separate launches reach wsc
]
# The candidates each case can run.  The second candidate of the 1x1 kind is the 1x1 GEMM weight
# gradient (conv._wgrad1x1_raw), which takes channel counts and pixel counts that are multiples
# of 16 only (bpk_gemm_nchw_wgrad_supported): the autograd nodes that record ("1x1",) pairs
# (conv._Conv and conv._ConvT of that kind, through conv1x1_ad) run for no other shape.  33 -> 17 channels at 5 x 5 therefore exists as a
# two-source launch alone, and 48 -> 32 at 4 x 4 is the smallest shape with both candidates.
W2_CANDIDATES = {"1x1_odd": (0,)}
# the choice nested under w2 = 1 (_wgrad_separate -> _wgrad_one) per case: a tag, or None
W2_NESTED = {"wino": "w3", "wino_pair": "w3", "igemm3x3": None, "1x1_odd": None, "1x1": None,
             "gen_k4s2": None, "gen_k3s2": None, "small_cout": "wsc"}

# every site in one second-order graph / the GroupNorm prologue form: N, Cin, Cout, H, W
SECOND_ORDER_CASE = (2, 32, 48, 8, 16)
GN_CASE = (2, 32, 48, 8, 16)
GN_GROUPS = 8


# ------------------------------------------------- the conditions of op/conv.py, by predicate
def _igemm(xshape, wshape, s=(1, 1), p=(1, 1)):
    from op import conv
    return bool(conv._igemm_shape_ok(tuple(xshape), tuple(wshape), tuple(s), tuple(p)))


def _small_img(H, W):
    from op import conv
    return H * W <= conv._SMALL_IMG_MAX_HW


def wino_fwd_form(N, cin, cout, H, W):
    """'wino', 'pair' or None: the Winograd forward kernel's form for conv3x3 of [N, cin, H, W]
    into cout channels"""
    from op.conv import lib
    if lib.bpk_conv3x3_wino_supported(N, cin, cout, H, W):
        return "wino"
    if lib.bpk_conv3x3_wino_pair_supported(N, cin, cout, H, W):
        return "pair"
    return None


def reaches_f3(N, cin, cout, H, W):
    return (wino_fwd_form(N, cin, cout, H, W) is not None and _small_img(H, W)
            and _igemm((N, cin, H, W), (cout, cin, 3, 3)))


def reaches_d3(N, c0, c1, H, W):
    """x [N, c0, H, W], w [c0, c1, 3, 3]: the result has c1 channels"""
    return (wino_fwd_form(N, c0, c1, H, W) is not None and _small_img(H, W)
            and _igemm((N, c1, H, W), (c0, c1, 3, 3)))


def reaches_w3(N, cin, cout, H, W):
    from op.conv import lib
    return (bool(lib.bpk_conv3x3_wino_wgrad_supported(N, cin, cout, H, W))
            and (_small_img(H, W) or cout % 64 != 0)
            and _igemm((N, cin, H, W), (cout, cin, 3, 3)))


def reaches_wsc(N, cin, cout, H, W, K):
    from op.conv import lib
    return (cout <= 4 and K in (1, 3)
            and bool(lib.bpk_conv2d_wgrad_small_cout_supported(N, cin, cout, H, W, K))
            and _igemm((N, cin, H, W), (cout, cin, K, K), (1, 1), (K // 2, K // 2)))


def reaches_dsc(N, cin, cout, H, W):
    from op.conv import lib
    return (cin <= 4 and bool(lib.bpk_conv3x3_small_supported(N, cout, cin, H, W))
            and _igemm((N, cin, H, W), (cout, cin, 3, 3)))


def w2_launch(kind, N1, N2, cin, cout, H, W, k, stride, pad):
    """'wino', 'igemm' or None: the two-source launch op.conv._two_source_ok finds for two
    pairs of equal shapes"""
    from op.conv import lib
    N = N1 + N2
    if kind[0] == "3x3" and lib.bpk_conv3x3_wino_wgrad_supported(N, cin, cout, H, W) \
            and (W != 8 or N1 % 2 == 0):
        return "wino"
    ok = _igemm((N, cin, H, W), (cout, cin, k, k), (stride, stride), (pad, pad))
    return "igemm" if ok else None
