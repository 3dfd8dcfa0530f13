"""LightGlue (csrc/lightglue.hip through the C ABI) at the keypoint counts where its tiles end, against oracle/lightglue_ref.py run on the CPU inside the test.

lg_flash / lg_flash_h work on 32-key blocks and 128-query workgroups, lg_kv_frags lays K and V out per 32-key block with a per-block operand scale, lg_sim uses
128 x 32 tiles, lg_lse / lg_best reduce columns in LG_CROWS = 32 row chunks that a second kernel folds, lg_gather compacts the sequences after pruning, and the
workspace is padded to MP = ceil(max_k / 128) * 128 and zeroed only when it grows.  The other files run 300/280, 1000, 1536 and 2048 points; this one runs

  count sweep   (1,1) (2,3) (1,40) (31,33) (32,32) (33,31) (5,200) (127,129) (128,128) (129,127) (257,96) (300,280): the smallest call, one query against a partial
                key block, either side of one 32-key block and of one 128-query workgroup, MP == max_k, very unequal sides, three workgroups against three key
                blocks, and the goldens' own count as an anchor.  Early stop and pruning off, the score filter open (depth_confidence = width_confidence = -1,
                filter_threshold = 0): all nine layers run at the full counts and EVERY mutual nearest pair comes back with its score, about 0.9 min(n0, n1) per
                case, down to scores of 1e-31.  256-dim weights (seed 21) at every count, 128-dim weights (seed 24, the input_proj path) up to (129,127).
  pruning       default conf, counts (40,36) (33,65) (70,20) (130,127) (200,160) with the "prune" weights (256-dim seed 23, 128-dim seed 25) and the "stop" weights
                (seed 22): the sequences shrink across the 32- and 128-boundaries mid-run, one side crossing while the other does not (asserted from the oracle's
                trace).  The (40,36) cases put points on the corners and edges of the image: the border taps of lg_sample.
  batch         ONE kpb_lg_match call of seven pairs (1,40) (33,31) (129,127) (5,200) (0,7) (7,0) (200,200), max_k = 200, the padding rows of the point buffers
                NaN: every pair bit for bit what the single-pair call gives; an empty side stops at 1, as the reference's loop does (it breaks before layer 0).
  dirty arena   (33,31) and (1,40) after (300,280) on one matcher (the workspace re-carved at MP = 128 over what MP = 384 left, no memset) against a fresh matcher,
                which then grows to (300,280) itself.
  strides       channels_last descriptor maps through lg_sample against the NCHW run.
  f16           attention="f16" at (1,40) (31,33) (33,31) (129,127) against the oracle fed half operands (refused with KPB_E_UNSUPPORTED under KPB_FP32_MATRIX=1).

Tolerances.  Pair sets must equal the fp32 oracle's; a pair in one set only is excused only if, in the FLOAT64 oracle's log_scores, the best and the second-best
entry of its row or of its column are less than 4e-3 apart (twice the score tolerance: a relative 2e-3 on a score is an absolute 2e-3 on its logarithm, and each of
the two candidates may move by that much), and never more than 2 % of the oracle's pairs.  Scores of common pairs: rtol 2e-3, atol 1e-5 against the fp32 oracle
(tests/test_gpu_lightglue.py).  With the filter open atol would wave the tiny scores through, so the sweep also compares log(score) of every common pair with the
float64 oracle by the rule of tests/test_gpu_net_shapes.py: e_ref = max |log s_fp32 - log s_fp64| is the reference arithmetic's own error on that case, and the GPU
passes if max |log s_gpu - log s_fp64| <= max(2e-3, 4 e_ref) (4: another summation order over K up to 512; a margin over the reference's error, never the GPU's).
The float64 oracle runs inside the test; no number is hard-coded.  f16: the bounds of the existing f16 test (pairs equal except within 2e-3 of the 0.1 threshold,
scores rtol 3e-3, atol 2e-5); the half-precision oracle agrees with the fp32 oracle on every pair at these four counts (seed 21, checked on the CPU).

Figures.  The oracle's own error on the CPU (e_ref, log-score domain), largest over the sweep: 256-dim 5.8e-4 at (127,129) on a smallest score of 6.6e-28; 128-dim
4.5e-3 at (31,33) on a smallest score of 6.8e-25; 8e-8 at (1,40); fp32 and float64 oracle agree on every pair of every case of the file, and the half-precision oracle
with the fp32 oracle at the four f16 counts.  The oracle's pruning runs, e.g. 256-dim (40,36) -> (35,32) -> (27,27) -> (24,26), stop 4; (130,127) -> (123,123) -> (83,87)
-> (70,71) -> (48,47), stop 9; 128-dim (40,36) -> (37,33) -> (32,30) -> (29,26), stop 9; "stop" weights: layer 3 at every count.  NOT YET MEASURED ON AN MI355X: the GPU's
score and log-score errors, the number of excused pairs (expected: none) and the run time, for the split-f16 form and for KPB_FP32_MATRIX=1 -- every test prints its
figures (pytest -s); the CPU side of the file (45 cases, both oracles) takes 18 s on a build machine.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from keypoint_bench_amd import weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMG = {"w": 320, "h": 240}
KPB_E_UNSUPPORTED = -7
STRICT = os.environ.get("KPB_FP32_MATRIX", "0") not in ("", "0")
FULL = dict(depth_confidence=-1, width_confidence=-1, filter_threshold=0.0)       # nine layers at the full counts, every mutual pair returned
DEFAULT = dict(depth_confidence=0.95, width_confidence=0.99, filter_threshold=0.1)
W256, W128 = (256, 8, "plain", 21), (128, 1, "plain", 24)                          # (dim, desc_scale, variant, weight seed)
COUNTS = [(1, 1), (2, 3), (1, 40), (31, 33), (32, 32), (33, 31), (5, 200), (127, 129), (128, 128), (129, 127), (257, 96), (300, 280)]
SWEEP = [(W256, c) for c in COUNTS] + [(W128, c) for c in COUNTS[:COUNTS.index((129, 127)) + 1]]
PRUNE_W = [(256, 8, "prune", 23), (256, 8, "stop", 22), (128, 1, "prune", 25)]
PRUNE_COUNTS = [(40, 36), (33, 65), (70, 20), (130, 127), (200, 160)]
F16_COUNTS = [(1, 40), (31, 33), (33, 31), (129, 127)]


def inputs(seed, dim, scale, n0, n1, H=240, W=320):
    g = np.random.default_rng(seed)
    Hd, Wd = H // scale, W // scale
    dm0 = g.normal(size=(1, dim, Hd, Wd)).astype(np.float32)
    dm1 = (dm0 + 0.25 * g.normal(size=dm0.shape)).astype(np.float32)
    mk = lambda n: np.concatenate([g.uniform(0.05, 0.95, size=(n, 2)), g.uniform(0.1, 1.0, size=(n, 1))], 1).astype(np.float32)
    p0 = mk(n0)
    ns = min(n0, n1) - min(n0, n1) // 5
    p1 = np.concatenate([p0[g.permutation(n0)[:ns]], mk(n1 - ns)], 0)[g.permutation(n1)]
    return dm0, dm1, p0, p1.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(w, n0, n1, border=False):
    dim, scale, _, seed = w
    dm0, dm1, p0, p1 = inputs(seed + n0 + n1, dim, scale, n0, n1)
    if border:      # the four corners and two edge midpoints: the border taps of lg_sample
        p0[:4, :2] = [[0, 0], [1, 1], [1, 0], [0, 1]]
        p1[:2, :2] = [[0, 0.5], [0.5, 1]]
    for a in (dm0, dm1, p0, p1):
        a.setflags(write=False)
    return dm0, dm1, p0, p1


@functools.lru_cache(maxsize=None)
def _tensors(w, double):
    dim, _, variant, seed = w
    t = weights.tensors_lightglue(weights.random_lightglue_state_dict(seed, dim, variant))
    return {k: torch.from_numpy(np.asarray(v)).double() if double else torch.from_numpy(np.asarray(v)) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _oracle(w, n0, n1, conf, double=False, half=False, border=False):
    """The plain torch restatement on the CPU, once per case for the whole file: {pair: score}, stop, the final log_scores with the index maps of their rows and
    columns, and the (m, n) the sequences had at every layer.  `half`: the caller has set lightglue_ref.HALF_ATTENTION (monkeypatch), checked here."""
    from oracle import lightglue_ref as R
    assert bool(R.HALF_ATTENTION) == half
    dm0, dm1, p0, p1 = _inputs(w, n0, n1, border)
    T = (lambda a: torch.from_numpy(a.copy()).double()) if double else (lambda a: torch.from_numpy(a.copy()))
    trace = []
    with torch.no_grad():
        _, _, out = R.match(_tensors(w, double), T(p0), T(p1), T(dm0), T(dm1), IMG, w[1], trace=trace, **dict(FULL if conf == "full" else DEFAULT))
    pairs = {tuple(r): float(s) for r, s in zip(out["matches"].numpy().tolist(), out["scores"].double().numpy().tolist())}
    return dict(pairs=pairs, stop=out["stop"], log_scores=out["log_scores"][0].double().numpy() if "log_scores" in out else None, ind0=trace[-1][2][0].numpy(), ind1=trace[-1][3][0].numpy(),
                sizes=[(t[0].shape[1], t[1].shape[1]) for t in trace])


def _matcher(w, conf, **kw):
    from keypoint_bench_amd.models.lightglue import LightGlue
    dim, scale, variant, seed = w
    m = LightGlue(features=None, desc_scale=scale, **kw, **conf)
    m.load_state_dict(weights.random_lightglue_state_dict(seed, dim, variant))
    return m


@functools.lru_cache(maxsize=None)
def _shared_matcher(w, conf):
    """One matcher per (weights, conf) for the whole file: it goes through every count in turn, as a caller's would."""
    return _matcher(w, dict(FULL if conf == "full" else DEFAULT))


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(m, w, n0, n1, border=False, maps=None):
    """(pairs [k,2] int64, scores [k] float32, stop) of one single-pair call, as numpy."""
    dm0, dm1, p0, p1 = _inputs(w, n0, n1, border)
    d0, d1 = maps if maps is not None else (_T(dm0), _T(dm1))
    pairs, scores, stop = m.match_indices(_T(p0), _T(p1), d0, d1, IMG)
    return pairs.cpu().numpy(), scores.cpu().numpy(), stop


def _margin(r64, pair):
    """Distance between the best and the second-best entry of the pair's row, or of its column if that is smaller, in the float64 oracle's log_scores."""
    a, b = np.nonzero(r64["ind0"] == pair[0])[0], np.nonzero(r64["ind1"] == pair[1])[0]
    if len(a) == 0 or len(b) == 0:
        return np.inf                                   # a point the float64 oracle pruned: nothing excuses it
    row, col = np.sort(r64["log_scores"][a[0], :]), np.sort(r64["log_scores"][:, b[0]])
    return min(row[-1] - row[-2] if len(row) > 1 else np.inf, col[-1] - col[-2] if len(col) > 1 else np.inf)


def _check(tag, got, r32, ref64, rtol=2e-3, atol=1e-5, log_rule=False):
    """Rules 1-6 of the module docstring on one result.  ref64() runs the float64 oracle; it is called only where a rule needs it."""
    pairs, scores, stop = got
    n0, n1 = tag[-1]
    assert stop == r32["stop"], (tag, stop, r32["stop"])
    assert np.all(np.diff(pairs[:, 0]) > 0), tag                                        # ascending in the first index, as torch.where leaves them
    assert np.all((pairs >= 0) & (pairs < np.array([n0, n1]))), tag
    assert np.all(np.isfinite(scores)) and np.all(scores > 0) and np.all(scores <= 1), (tag, scores.min() if len(scores) else None)
    gs = {tuple(r): float(s) for r, s in zip(pairs.tolist(), scores.tolist())}
    ws = r32["pairs"]
    assert len(gs) == len(pairs), tag
    diff = sorted(set(gs) ^ set(ws))
    r64 = ref64() if (diff or log_rule) else None
    for r in diff:
        mg = _margin(r64, r)
        assert mg < 4e-3, "%s: pair %s is in one set only and the float64 oracle separates it from the runner-up by %.3g" % (tag, r, mg)
    assert len(diff) <= 0.02 * len(ws), (tag, diff)
    common = sorted(set(gs) & set(ws))
    g_, w_ = np.array([gs[r] for r in common]), np.array([ws[r] for r in common])
    rel = float(np.max(np.abs(g_ - w_) / w_)) if common else 0.0
    line = "%s: %d pairs, %d excused, max rel score error %.3g" % (tag, len(ws), len(diff), rel)
    if log_rule:
        w64 = r64["pairs"]
        e_ref = max([abs(np.log(ws[r]) - np.log(w64[r])) for r in set(ws) & set(w64)], default=0.0)
        e_gpu = max([abs(np.log(gs[r]) - np.log(w64[r])) for r in common if r in w64], default=0.0)
        line += ", log-score error %.3g (e_ref %.3g, min score %.3g, oracle fp32 / fp64 pair sets differ by %d)" % (e_gpu, e_ref, min(ws.values()), len(set(ws) ^ set(w64)))
    print(line)
    np.testing.assert_allclose(g_, w_, rtol=rtol, atol=atol, err_msg=str(tag))
    if log_rule:
        assert e_gpu <= max(2e-3, 4 * e_ref), (tag, e_gpu, e_ref)
    return len(diff)


def _wname(w):
    return "%d%s" % (w[0], w[2])


@pytest.mark.parametrize("w,cnt", SWEEP, ids=["%s-%dx%d" % (_wname(w), c[0], c[1]) for w, c in SWEEP])
def test_every_layer_and_every_mutual_pair_at_the_tile_edges(w, cnt):
    n0, n1 = cnt
    got = _run(_shared_matcher(w, "full"), w, n0, n1)
    assert got[2] == 9
    _check((_wname(w), "strict fp32" if STRICT else "split-f16", cnt), got, _oracle(w, n0, n1, "full"), lambda: _oracle(w, n0, n1, "full", double=True), log_rule=True)


PRUNE = [(w, c) for w in PRUNE_W for c in PRUNE_COUNTS]


@pytest.mark.parametrize("w,cnt", PRUNE, ids=["%s-%dx%d" % (_wname(w), c[0], c[1]) for w, c in PRUNE])
def test_pruning_and_early_stop_across_tile_boundaries(w, cnt):
    n0, n1 = cnt
    border = cnt == (40, 36)
    r32 = _oracle(w, n0, n1, "default", border=border)
    sizes = r32["sizes"]
    if w[2] == "prune":     # the case is here for sequences that shrink across a 32-boundary: a change of the weights helper must not quietly end that
        assert sizes[-1][0] < n0 and sizes[-1][1] < n1, sizes
        blocks = [((a + 31) // 32, (b + 31) // 32) for a, b in sizes]
        assert any(x != y for x, y in zip(blocks, blocks[1:])), sizes
    else:
        assert r32["stop"] < 9, r32["stop"]
    got = _run(_matcher(w, DEFAULT, prune_min_kpts=-1), w, n0, n1, border)
    print("%s %s: oracle sizes %s stop %d" % (_wname(w), cnt, sizes, r32["stop"]))
    _check((_wname(w), "strict fp32" if STRICT else "split-f16", cnt), got, r32, lambda: _oracle(w, n0, n1, "default", double=True, border=border))


BATCH = [(1, 40), (33, 31), (129, 127), (5, 200), (0, 7), (7, 0), (200, 200)]


def _batch_call(m, cases, K):
    """One kpb_lg_match call over `cases` = [(dm0, dm1, p0, p1)], the point buffers padded to K rows with NaN.  Returns per pair (pairs, score bits, stop)."""
    from keypoint_bench_amd._lib import LgParams, ptr
    dev = torch.device(DEV)
    B = len(cases)
    P0 = torch.full((B, K, 3), float("nan"), device=dev); P1 = torch.full((B, K, 3), float("nan"), device=dev)
    for b, (_, _, p0, p1) in enumerate(cases):
        if len(p0):
            P0[b, : len(p0)] = _T(p0)
        if len(p1):
            P1[b, : len(p1)] = _T(p1)
    D0 = torch.stack([_T(c[0])[0] for c in cases]).contiguous(); D1 = torch.stack([_T(c[1])[0] for c in cases]).contiguous()
    n0 = torch.tensor([len(c[2]) for c in cases], dtype=torch.int32, device=dev); n1 = torch.tensor([len(c[3]) for c in cases], dtype=torch.int32, device=dev)
    pairs = torch.full((B, K, 2), -1, dtype=torch.int32, device=dev); scores = torch.full((B, K), float("nan"), dtype=torch.float32, device=dev)
    k = torch.full((B,), -1, dtype=torch.int32, device=dev); stop = torch.full((B,), -1, dtype=torch.int32, device=dev)
    _, C, Hd, Wd = D0.shape
    sb, sc, sh, sw = D0.stride()
    prm = LgParams(float(m.conf["depth_confidence"]), float(m.conf["width_confidence"]), float(m.conf["filter_threshold"]), m.prune_min_kpts)
    ctx = m._ctx
    ctx.check(ctx.lib.kpb_lg_match(m._handle, ptr(P0), ptr(P1), ptr(n0), ptr(n1), B, K, ptr(D0), ptr(D1), C, Hd, Wd, sb, sc, sh, sw, IMG["w"], IMG["h"],
                                   ctypes.byref(prm), ptr(pairs), ptr(scores), ptr(k), ptr(stop)))
    out = []
    for b in range(B):
        kb = int(k[b])
        assert 0 <= kb <= K, (b, kb)
        out.append((pairs[b, :kb].cpu().numpy(), scores[b, :kb].cpu().numpy().view(np.uint32), int(stop[b])))
    return out


@pytest.mark.parametrize("w,conf", [(W256, "full"), ((256, 8, "prune", 23), "default")], ids=["plain-full", "prune-default"])
def test_one_batch_of_very_different_pairs_equals_the_single_pair_calls(w, conf):
    """Seven pairs of 1 to 200 points in one call, two of them with an empty side, the padding NaN: same kernels, same per-pair arithmetic as the single-pair call
    on the same matcher, so pairs, score bits, stop and k are equal bit for bit and nothing past n is read into a result."""
    m = _matcher(w, dict(FULL if conf == "full" else DEFAULT))
    cases = []
    for n0, n1 in BATCH:
        dm0, dm1, p0, p1 = _inputs(w, max(n0, 1), max(n1, 1))      # (the generator cannot make an empty side: one point, dropped)
        cases.append((dm0, dm1, p0[:n0], p1[:n1]))
    singles = []
    for dm0, dm1, p0, p1 in cases:
        sp, ss, st = m.match_indices(_T(p0), _T(p1), _T(dm0), _T(dm1), IMG)
        singles.append((sp.cpu().numpy(), ss.cpu().numpy().view(np.uint32), st))
    # the comparison below is not one of empty results: the single-pair calls return what the oracle does on the five pairs it can run
    want = sum(len(_oracle(w, n0, n1, conf)["pairs"]) for n0, n1 in BATCH if n0 and n1)
    assert want >= 40 and sum(len(s[0]) for s in singles) >= 0.98 * want, (want, [len(s[0]) for s in singles])
    for (n0, n1), (sp, ss, st) in zip(BATCH, singles):              # ... pair for pair, scores and stop layer included
        if n0 and n1:
            _check((_wname(w), "strict fp32" if STRICT else "split-f16", (n0, n1)), (sp, ss.view(np.float32), st), _oracle(w, n0, n1, conf),
                   lambda: _oracle(w, n0, n1, conf, double=True))
    if conf == "default":       # (1,40) loses its only point of side 0 to the pruning of layer 2: the reference leaves its loop before layer 3 and returns i + 1 = 4, no match
        assert _oracle(w, 1, 40, conf)["sizes"][-1][0] == 1 and _oracle(w, 1, 40, conf)["stop"] == 4 and singles[0][2] == 4 and len(singles[0][0]) == 0
    batch = _batch_call(m, cases, 200)
    for b, ((sp, ss, st), (bp, bs, bst)) in enumerate(zip(singles, batch)):
        assert bst == st, (BATCH[b], bst, st)
        np.testing.assert_array_equal(bp, sp.astype(np.int32), err_msg="pair %d %s" % (b, BATCH[b]))
        np.testing.assert_array_equal(bs, ss, err_msg="pair %d %s" % (b, BATCH[b]))
    # an empty side: no match, and the layer count the reference's loop leaves -- it breaks before layer 0 with i = 0 and returns i + 1
    # (lightglue.py:553-554; oracle/lightglue_ref.py forward: `if desc0.shape[1] == 0 or desc1.shape[1] == 0: break` ... `stop=i + 1`)
    for b in (BATCH.index((0, 7)), BATCH.index((7, 0))):
        assert len(batch[b][0]) == 0 and len(singles[b][0]) == 0
        assert batch[b][2] == 1 and singles[b][2] == 1, (batch[b][2], singles[b][2])


def _bits(got):
    return got[0].tolist(), got[1].view(np.uint32).tolist(), got[2]


def test_a_small_call_on_the_workspace_a_large_call_left_dirty():
    """The workspace is zeroed only when it grows.  After (300,280) it is carved for MP = 384 and full of that call's values -- integers (index maps, 0x7FFFFFFF
    "no winner" marks, -1 "pruned" marks: NaN bit patterns) as much as floats; (33,31) and (1,40) re-carve it at MP = 128 without a memset, so their padded rows and
    their partial arrays hold whatever lies there.  A fresh matcher's workspace is all zeros.  The two must agree bit for bit, and the large call must still
    reproduce itself afterwards.  The other direction: the fresh matcher, carved at MP = 128 by its two small calls, then runs (300,280), which reserves the
    workspace again at MP = 384 and zero-fills it; it must give the first matcher's bits."""
    w = W256
    a = _matcher(w, FULL)
    first = _bits(_run(a, w, 300, 280))
    small_dirty = [_bits(_run(a, w, n0, n1)) for n0, n1 in ((33, 31), (1, 40))]
    b = _matcher(w, FULL)
    small_fresh = [_bits(_run(b, w, n0, n1)) for n0, n1 in ((33, 31), (1, 40))]
    assert len(small_fresh[0][0]) >= 20 and len(small_fresh[1][0]) == 1
    assert small_dirty == small_fresh
    assert _bits(_run(a, w, 300, 280)) == first
    assert _bits(_run(b, w, 300, 280)) == first


def test_channels_last_descriptor_maps_through_lg_sample():
    """lg_sample takes element strides (kpb_sample has its own such test; this is a separate kernel): NHWC maps give the NCHW run's pairs and score bits."""
    w, (n0, n1) = W256, (129, 127)
    m = _shared_matcher(w, "full")
    dm0, dm1, _, _ = _inputs(w, n0, n1)
    cl = tuple(_T(d).contiguous(memory_format=torch.channels_last) for d in (dm0, dm1))
    assert cl[0].stride(1) == 1 and cl[0].stride(3) == w[0]
    want, got = _bits(_run(m, w, n0, n1)), _bits(_run(m, w, n0, n1, maps=cl))
    assert len(want[0]) > 90
    assert got == want


@pytest.mark.parametrize("cnt", F16_COUNTS, ids=["%dx%d" % c for c in F16_COUNTS])
def test_f16_attention_at_the_tile_edges(cnt, monkeypatch):
    from keypoint_bench_amd._lib import KpbError
    from oracle import lightglue_ref as R
    w, (n0, n1) = W256, cnt
    m = _matcher(w, DEFAULT, attention="f16")
    if STRICT:          # the strict-fp32 build has no f16 attention: the first call says so
        with pytest.raises(KpbError) as e:
            _run(m, w, n0, n1)
        assert e.value.code == KPB_E_UNSUPPORTED
        return
    monkeypatch.setattr(R, "HALF_ATTENTION", True)
    ref = _oracle(w, n0, n1, "default", half=True)
    pairs, scores, stop = _run(m, w, n0, n1)
    assert stop == ref["stop"]
    assert np.all(np.diff(pairs[:, 0]) > 0)
    ws, gs = ref["pairs"], {tuple(r): float(s) for r, s in zip(pairs.tolist(), scores.tolist())}
    for r in set(ws) ^ set(gs):
        s = ws.get(r, gs.get(r))
        assert abs(s - 0.1) < 2e-3, "%s: match %s (score %.4f) differs and is not at the threshold" % (cnt, r, s)
    common = sorted(set(ws) & set(gs))
    assert len(common) >= 0.98 * len(ws) and len(common) > 0
    g_, w_ = np.array([gs[r] for r in common]), np.array([ws[r] for r in common])
    print("f16 %s: %d pairs, %d at the threshold, max rel score error %.3g" % (cnt, len(ws), len(set(ws) ^ set(gs)), np.max(np.abs(g_ - w_) / w_)))
    np.testing.assert_allclose(g_, w_, rtol=3e-3, atol=2e-5)
