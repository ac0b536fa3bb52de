"""pp_decode_nms_batch_dev on every path its candidate sort can take, on exact score ties, on non-finite
class logits, on the full width of the key's anchor-id field and at an IoU equal to the threshold --
against tests/nms_restatement.py.  Bars as in tests/test_gpu_postprocess.py: count, kept anchor ids, their
order and the class column exact, padding exact, decoded rows within 1e-5.

The inputs are synthetic and exact (see Case): one anchor per cell, integer rectangles, so every f32 area,
intersection and ratio is exact; candidate logits are -level * 2^-15 (level < 2^18), whose f64 sigmoids lie
more than 16 f32 ulps apart, so the candidate order does not depend on whose expf is used; ties are made
with bit-identical logits only.  Two designs look into the order:

  shallow  disjoint rectangles, nothing is suppressed: the output is the first max_out candidates;
  deep     all candidates share ONE rectangle, except a set of witnesses with disjoint rectangles of
           their own, at ranks scattered through the whole order: with nms_thresh 0.5 the output is the
           witnesses plus the best member of the shared group, in rank order -- k_nms walks every chunk
           and carries its kept list across all of them.

test_generators_and_restatement needs no device: it checks what the GPU tests lean on (score gaps, tie
bits, the candidate count and sort path of every case, and that the restatement gives the closed-form
expectation).  The references are computed once per case and shared.
"""
import ctypes
import functools
import types

import numpy as np
import pytest

import nms_restatement as N

# csrc/pp_decode.hip: kRun (candidates per sorted run), kMaxRuns (runs merged on the fly), kChunkN
# (candidates per NMS chunk)
K_RUN, K_MAX_RUNS, K_CHUNK = 16384, 8, 256
ONE_RUN, MERGED, IN_PLACE = "one run", "merged runs", "in place"

BIG = (363, 363)                    # A = 131769: cap = 2^18, more than kMaxRuns * kRun candidates fit
A_BIG = BIG[0] * BIG[1]
STEP, ORIGIN = 0.25, -10.0          # x_step = y_step, x_min = y_min
BACKGROUND = -30.0                  # logit of a non-candidate
POS_THRESH = 1e-4
MIN_GAP_ULPS = 16
RANKS = (0, 255, 256, 257, 16383, 16384, 16385, 131071, 131072, 131073)   # always witnesses, where they exist


def sort_path(M, A):
    """The path pp_decode_nms_batch_dev takes for M candidates of A anchors."""
    cap = 1
    while cap < A:
        cap <<= 1
    run = min(K_RUN, cap)
    if M <= run:
        return ONE_RUN
    return MERGED if M <= K_MAX_RUNS * run else IN_PLACE


def level_logits(level):
    """-level * 8 / 2^18 as f32: exact for level < 2^18."""
    level = np.asarray(level, np.int64)
    assert level.size == 0 or (0 <= level.min() and level.max() < 2 ** 18)
    out = (-(level.astype(np.float64) * 8.0 / 2 ** 18)).astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * 2 ** 15, -level)
    return out


class Sample:
    """One sample's candidates: ``order`` anchor ids by rank (rank 0 is best), ``logits`` their maximal
    class logit (f32, non-increasing; equal logits = a tie, ids ascending inside it), ``klass`` the class
    that must be reported; ``cls`` [C, A] all class logits."""

    def __init__(self, A, order, logits, num_classes=1, klass=None, background=BACKGROUND):
        self.order = np.asarray(order, np.int64)
        self.logits = np.asarray(logits, np.float32)
        self.klass = np.zeros(len(self.order), np.int64) if klass is None else np.asarray(klass, np.int64)
        self.cls = np.full((num_classes, A), background, np.float32)
        self.cls[self.klass, self.order] = self.logits

    @property
    def M(self):
        return len(self.order)


class Case:
    """``fm`` feature map (one anchor per cell), ``samples``, ``own``: ids of the anchors that keep their own
    disjoint unit square (None: all of them -- the shallow design); every other anchor gets the one shared
    rectangle.  ``rects`` overrides single rectangles (x1, y1, x2, y2 in the kernel's flipped frame).
    ``expected`` (per sample) is the closed-form kept list."""

    def __init__(self, fm, samples, own=None, rects=None, max_out=1024, nms_thresh=0.5, pos_thresh=POS_THRESH,
                 nms="anchor", class_aware=False, path=None, reg_seed=None, expected=None, expected_classes=None):
        self.fm, self.samples = fm, samples
        self.Hf, self.Wf = fm
        self.A = self.Hf * self.Wf
        self.C = samples[0].cls.shape[0]
        self.max_out, self.nms_thresh, self.pos_thresh = max_out, nms_thresh, pos_thresh
        self.nms, self.class_aware, self.path = nms, class_aware, path
        self.H = 2 * max(fm) + 64              # canvas height: room for the shared and the special rectangles
        self.own = None if own is None else np.asarray(own, np.int64)
        self.own_mask = np.ones(self.A, bool)
        if own is not None:
            self.own_mask[:] = False
            self.own_mask[self.own] = True
        iy, ix = np.divmod(np.arange(self.A), self.Wf)
        x1, y1 = 2.0 * ix, 2.0 * iy           # unit squares on a pitch of 2, in the flipped frame
        box = np.stack([x1, y1, x1 + 1, y1 + 1], 1)
        box[~self.own_mask] = [2 * self.Wf + 2, 0, 2 * self.Wf + 3, 1]
        for a, r in (rects or {}).items():
            box[a] = r
        xy = box.copy()                       # stored so that the kernel's (canvas_height-1) - y gives box back
        xy[:, 1], xy[:, 3] = (self.H - 1) - box[:, 1], (self.H - 1) - box[:, 3]
        self.anchors = dict(centers=np.stack([x1 + 0.5, (self.H - 1) - (y1 + 0.5), np.zeros(self.A)], 1),
                            wlh=np.ones((self.A, 3)), yaw=np.zeros(self.A), xy=xy)
        self.reg = np.zeros((len(samples), 8, self.A), np.float32)
        if reg_seed is not None:              # decoded rows that differ: small offsets at the witnesses
            rng = np.random.default_rng(reg_seed)
            ids = np.arange(self.A) if own is None else self.own[:2048]
            self.reg[:, :, ids] = rng.normal(0, 0.1, (len(samples), 8, len(ids))).astype(np.float32)
        self.expected = expected if expected is not None else [self._closed_form(s) for s in samples]
        self.expected_classes = expected_classes

    def _closed_form(self, s):
        keep = self.own_mask[s.order]
        shared = np.nonzero(~keep)[0]
        if len(shared):
            if self.class_aware:               # the best member of the shared group of every class
                _, first = np.unique(s.klass[shared], return_index=True)
                keep[shared[first]] = True
            else:
                keep[shared[0]] = True
        return s.order[keep][:self.max_out]

    @property
    def geometry(self):
        return self.H, STEP, STEP, ORIGIN, ORIGIN

    def cls_tensor(self, b):
        return self.samples[b].cls.reshape(self.C, self.Hf, self.Wf)

    def reg_tensor(self, b):
        return self.reg[b].reshape(8, self.Hf, self.Wf)


# ---- generators -------------------------------------------------------------------------------------

def _witness_ranks(M, n, rng):
    """The ranks that are always witnesses, the last two, and n random ones."""
    must = [r for r in RANKS + (M - 2, M - 1) if 0 <= r < M]
    extra = rng.choice(M, min(M, n), replace=False)
    return np.unique(np.concatenate([must, extra]).astype(np.int64))


def _deep(fm, M, seed, n_wit=250, **kw):
    rng = np.random.default_rng(seed)
    A = fm[0] * fm[1]
    order = rng.permutation(A)[:M]
    ranks = _witness_ranks(M, n_wit, rng)
    return Case(fm, [Sample(A, order, level_logits(np.arange(M)))], own=order[ranks], reg_seed=seed,
                path=sort_path(M, A), **kw)


def _shallow(fm, M, seed, top="random", reg=True, **kw):
    """top: which anchor ids get the best ranks -- 'random', the 'highest' ids (the last, partial run: k_score
    appends roughly in id order) or the 'lowest'."""
    rng = np.random.default_rng(seed)
    A = fm[0] * fm[1]
    order = rng.permutation(A)[:M]
    if top != "random":
        ids = np.sort(order)
        head = ids[::-1][:2000] if top == "highest" else ids[:2000]
        rest = np.setdiff1d(ids, head)
        order = np.concatenate([head, rng.permutation(rest)])
    return Case(fm, [Sample(A, order, level_logits(np.arange(M)))], reg_seed=seed if reg else None,
                path=sort_path(M, A), **kw)


def _class_aware(seed=5):
    rng = np.random.default_rng(seed)
    order = rng.permutation(A_BIG)
    klass = rng.integers(0, 2, A_BIG)
    ranks = _witness_ranks(A_BIG, 250, rng)
    return Case(BIG, [Sample(A_BIG, order, level_logits(np.arange(A_BIG)), 2, klass)], own=order[ranks],
                class_aware=True, reg_seed=seed, path=IN_PLACE)


def _tie_levels(M, groups):
    level = np.arange(M)
    for lo, hi in groups:
        level[lo:hi] = lo
    return level


def _sort_ties(order, logits):
    """ids ascending inside every group of equal logits"""
    order = order.copy()
    start = np.concatenate([[0], np.nonzero(logits[1:] != logits[:-1])[0] + 1, [len(order)]])
    for lo, hi in zip(start[:-1], start[1:]):
        if hi - lo > 1:
            order[lo:hi] = np.sort(order[lo:hi])
    return order


TIE_GROUPS = ((250, 262), (16380, 16390), (30000, 70000), (131068, 131078))


def _ties_deep(M, seed=7):
    """Tie groups across a chunk, a run, 131072, and one of 40000 equal scores; the witnesses sit inside them."""
    rng = np.random.default_rng(seed)
    groups = [g for g in TIE_GROUPS if g[1] <= M]
    logits = level_logits(_tie_levels(M, groups))
    order = _sort_ties(rng.permutation(A_BIG)[:M], logits)
    ranks = [np.arange(lo, hi) for lo, hi in groups if hi - lo < 100]
    ranks += [np.array([30000, 30001, 32767, 32768, 32769, 49151, 49152, 65535, 65536, 69998, 69999]),
              rng.integers(30000, 70000, 150), _witness_ranks(M, 60, rng)]
    ranks = np.unique(np.concatenate(ranks))
    return Case(BIG, [Sample(A_BIG, order, logits)], own=order[ranks], reg_seed=seed, path=sort_path(M, A_BIG))


def _ties_top(seed=8):
    """600 saturated scores (logit 20: sigmoid == 1.0f for everyone) at the top, ids over the whole range."""
    rng = np.random.default_rng(seed)
    logits = level_logits(np.arange(A_BIG))
    logits[:600] = 20.0
    order = rng.permutation(A_BIG)
    order[:600] = np.sort(order[:600])
    return Case(BIG, [Sample(A_BIG, order, logits)], reg_seed=seed, path=IN_PLACE)


def _ties_classes(seed=9):
    """A = 4096, 9 classes: every third candidate holds its maximal logit in two classes; the lower is reported."""
    rng = np.random.default_rng(seed)
    fm, A, M = (64, 64), 4096, 300
    order = rng.permutation(A)[:M]
    klass = rng.integers(0, 8, M)
    s = Sample(A, order, level_logits(np.arange(M)), 9, klass)
    twin = np.arange(0, M, 3)
    other = np.array([rng.integers(k + 1, 9) for k in klass[twin]])
    s.cls[other, order[twin]] = s.logits[twin]                     # bit-identical, at a higher class index
    lower = np.arange(1, M, 3)                                      # and a lower logit in another class
    s.cls[(klass[lower] + 1) % 9, order[lower]] = s.logits[lower] - np.float32(1.0)
    return Case(fm, [s], reg_seed=seed, path=ONE_RUN, expected_classes=[klass])


def _nonfinite(nms, seed=10):
    """9 classes, pos_thresh 0 (the background logit -100 has score exactly 0).  Rule: an anchor with a NaN
    score in any class is no candidate; +inf is the score 1.0; -inf the score 0."""
    rng = np.random.default_rng(seed)
    fm, A, M = (64, 64), 4096, 300
    ids = rng.permutation(A)
    order, special = ids[:M], ids[M:M + 20]
    klass = rng.integers(0, 9, M)
    s = Sample(A, order, level_logits(np.arange(M) + 10), 9, klass, background=-100.0)
    s.cls[(klass[::4] + 3) % 9, order[::4]] = -np.inf                # candidates all the same
    s.cls[(klass[1::4] + 5) % 9, order[1::4]] = s.logits[1::4] - np.float32(2.0)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = special
    s.cls[2, a[0]], s.cls[6, a[0]] = nan, 5.0                         # one NaN class beside a class at +5
    s.cls[6, a[1]], s.cls[2, a[1]] = nan, 5.0                         # ... the NaN after the maximum
    s.cls[0, a[2]], s.cls[8, a[2]] = nan, 5.0
    s.cls[:, a[3]] = nan                                              # all classes NaN
    s.cls[:, a[4]] = nan
    s.cls[4, a[5]] = inf                                              # score exactly 1.0: candidates
    s.cls[0, a[6]] = inf
    s.cls[8, a[7]], s.cls[1, a[7]] = inf, 20.0                        # 1.0 twice: the lower class
    s.cls[3, a[8]] = -inf                                             # score 0: not above pos_thresh 0
    s.cls[:, a[9]] = -inf
    s.cls[5, a[10]] = -100.0
    s.cls[1, a[11]], s.cls[7, a[11]] = -1.0, nan                      # NaN in a class that is not the maximum
    s.cls[7, a[12]], s.cls[1, a[12]] = -2.0, nan
    s.cls[3, a[13]], s.cls[4, a[13]], s.cls[5, a[13]] = nan, 20.0, inf
    s.cls[0, a[14]], s.cls[8, a[14]] = -inf, nan
    top = np.sort(a[5:8])                                             # three scores 1.0: by ascending id
    top_class = {int(a[5]): 4, int(a[6]): 0, int(a[7]): 1}
    s.order = np.concatenate([top, order])
    s.logits = np.concatenate([np.full(3, inf, np.float32), s.logits])
    s.klass = np.concatenate([[top_class[int(t)] for t in top], klass])
    case = Case(fm, [s], pos_thresh=0.0, nms=nms, path=ONE_RUN, expected_classes=[s.klass])
    case.nan_ids = np.sort(np.concatenate([a[:5], a[11:15]]))
    return case


def _id_width():
    """A = 2^20 - 1: the 300 highest and the 300 lowest anchor ids, ranks interleaved."""
    fm = (1023, 1025)
    A = fm[0] * fm[1]
    assert A == 2 ** 20 - 1
    order = np.stack([A - 1 - np.arange(300), np.arange(300)], 1).reshape(-1)
    return Case(fm, [Sample(A, order, level_logits(np.arange(600)))], reg_seed=11, path=ONE_RUN)


HALF, DUP, ZERO = "iou 0.5", "duplicate", "zero area"
# (rank of the first, rank of the second, kind): inside one chunk, and split across chunk boundaries
# (the second then meets the first in the kept list)
PAIRS = ((10, 11, HALF), (20, 25, DUP), (30, 31, ZERO), (300, 310, HALF), (250, 256, HALF), (251, 270, DUP),
         (252, 513, ZERO), (253, 600, HALF), (511, 512, DUP), (255, 699, DUP), (40, 520, HALF))


def _equal(below):
    """IoU exactly nms_thresh: [0,0,3,1] and [1,0,4,1] intersect in 2 of a union of 4.  nms_thresh 0.5 keeps
    both (strict >); the f32 just below 0.5 drops the second.  Duplicates go either way; 0/0 is NaN: kept."""
    fm, A, M = (32, 32), 1024, 700
    order = np.random.default_rng(12).permutation(A)[:M]
    thr = float(np.nextafter(np.float32(0.5), np.float32(0))) if below else 0.5
    rects, dropped = {}, []
    for k, (i, j, kind) in enumerate(PAIRS):
        y = 2 * fm[0] + 2 + 2 * k
        first, second = {HALF: ([0, y, 3, y + 1], [1, y, 4, y + 1]), DUP: ([0, y, 1, y + 1], [0, y, 1, y + 1]),
                         ZERO: ([5, y, 5, y], [5, y, 5, y])}[kind]
        rects[int(order[i])], rects[int(order[j])] = first, second
        if kind == DUP or (kind == HALF and below):
            dropped.append(j)
    case = Case(fm, [Sample(A, order, level_logits(np.arange(M)))], rects=rects, nms_thresh=thr, path=ONE_RUN,
                expected=[np.delete(order, dropped)])
    assert case.H - 1 >= 2 * fm[0] + 2 + 2 * len(PAIRS) + 1
    return case


BATCH_M = (0, 300, 40000, A_BIG)


def _batch(seed=13):
    """Four samples over one anchor set: no candidate, one run, merged runs, in place; deep design (the
    witnesses are anchors, so every sample sees those of them that are among its candidates)."""
    rng = np.random.default_rng(seed)
    full = rng.permutation(A_BIG)
    own = full[_witness_ranks(A_BIG, 400, rng)]
    samples = []
    for M in BATCH_M:
        order = full if M == A_BIG else rng.permutation(np.concatenate([own[:60], full[~np.isin(full, own[:60])]])[:M])
        samples.append(Sample(A_BIG, order, level_logits(np.arange(M))))
    return Case(BIG, samples, own=own, reg_seed=seed)


BOUNDARY_PATHS = {1: ONE_RUN, 255: ONE_RUN, 256: ONE_RUN, 257: ONE_RUN, 16383: ONE_RUN, 16384: ONE_RUN,
                  16385: MERGED, 32768: MERGED, 32769: MERGED, 131071: MERGED, 131072: MERGED,
                  131073: IN_PLACE, A_BIG: IN_PLACE}
POW2 = {16384: ((128, 128), ONE_RUN), 32768: ((128, 256), MERGED), 131072: ((512, 256), MERGED)}

CASES = {}
for _M, _p in BOUNDARY_PATHS.items():
    CASES[f"deep-{_M}"] = (functools.partial(_deep, BIG, _M, 100 + _M % 97, n_wit=985 if _M == A_BIG else 250), _p)
for _M in (16385, 131073, A_BIG):
    CASES[f"shallow-{_M}"] = (functools.partial(_shallow, BIG, _M, 200 + _M % 97), BOUNDARY_PATHS[_M])
CASES["shallow-highest-40000"] = (functools.partial(_shallow, BIG, 40000, 31, "highest"), MERGED)
CASES["shallow-lowest-40000"] = (functools.partial(_shallow, BIG, 40000, 32, "lowest"), MERGED)
CASES[f"shallow-highest-{A_BIG}"] = (functools.partial(_shallow, BIG, A_BIG, 33, "highest"), IN_PLACE)
for _A, (_fm, _p) in POW2.items():
    CASES[f"pow2-{_A}"] = (functools.partial(_deep, _fm, _A, 300 + _A % 97), _p)
CASES["class-aware"] = (_class_aware, IN_PLACE)
CASES["rotated"] = (functools.partial(_shallow, BIG, A_BIG, 41, reg=False, nms="rotated", max_out=256), IN_PLACE)
CASES["ties-deep"] = (functools.partial(_ties_deep, A_BIG), IN_PLACE)
CASES["ties-deep-merged"] = (functools.partial(_ties_deep, 100000), MERGED)
CASES["ties-top"] = (_ties_top, IN_PLACE)
CASES["ties-classes"] = (_ties_classes, ONE_RUN)
CASES["nonfinite-anchor"] = (functools.partial(_nonfinite, "anchor"), ONE_RUN)
CASES["nonfinite-rotated"] = (functools.partial(_nonfinite, "rotated"), ONE_RUN)
CASES["id-width"] = (_id_width, ONE_RUN)
CASES["equal-at"] = (functools.partial(_equal, False), ONE_RUN)
CASES["equal-below"] = (functools.partial(_equal, True), ONE_RUN)
CASES["batch"] = (_batch, None)


def make_case(name):
    build, path = CASES[name]
    case = build()
    if path is not None:                 # the path the case is meant for is the one its M gives
        assert case.path == path == sort_path(case.samples[0].M, case.A), (name, case.path, path)
    return case


@functools.lru_cache(maxsize=None)
def reference(name):
    """``[(boxes, kept ids, margin)]`` per sample from the restatement -- once per case."""
    case = make_case(name)
    out = []
    for b in range(len(case.samples)):
        out.append(N.postprocess(case.cls_tensor(b), case.reg_tensor(b), case.anchors, *case.geometry,
                                 pos_thresh=case.pos_thresh, nms_thresh=case.nms_thresh, max_out=case.max_out,
                                 num_classes=case.C, nms=case.nms, class_aware=case.class_aware))
    return out


# ---- the CPU part -----------------------------------------------------------------------------------

def _sigmoid(x):
    """f64 sigmoid of f32 logits.  A logit of -90 or less is the score 0: expf(90) overflows f32 in any libm."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.where(x <= -90.0, 0.0, 1.0 / (1.0 + np.exp(-x)))


def _check_sample(case, s):
    """The preconditions the GPU tests lean on; returns the number of tied neighbours."""
    thr = float(np.float32(case.pos_thresh))
    has_nan = np.isnan(s.cls).any(0)
    scores = _sigmoid(np.where(np.isnan(s.cls), -np.inf, s.cls))
    best = np.where(has_nan, 0.0, scores.max(0))
    # the candidates are exactly `order`, with the maximal logit `logits` and its first class `klass`
    assert np.array_equal(np.sort(s.order), np.nonzero(best > thr)[0]) and len(np.unique(s.order)) == s.M
    assert np.array_equal(s.cls[:, s.order].max(0), s.logits)
    assert np.array_equal(scores[:, s.order].astype(np.float32).argmax(0), s.klass)
    # nobody sits near the threshold: the candidates 16 ulps above it, the others at 0 or a factor 1000 below
    score = _sigmoid(s.logits)
    if s.M:
        assert score.min() - thr >= MIN_GAP_ULPS * np.spacing(np.float32(max(thr, 1e-30)))
    rest = np.delete(best, s.order)
    assert rest.size == 0 or rest.max() <= thr * 1e-3
    # decreasing scores at least 16 f32 ulps apart, or bit-identical logits with ascending ids
    tie = s.logits[1:].view(np.uint32) == s.logits[:-1].view(np.uint32)
    assert (s.logits[1:] <= s.logits[:-1]).all() and np.array_equal(tie, s.logits[1:] == s.logits[:-1])
    saturated = (score[1:] == 1.0) & (score[:-1] == 1.0)            # +inf and 20: 1.0f on every libm, a tie as well
    ulps = (score[:-1] - score[1:]) / np.spacing(score[:-1].astype(np.float32)).astype(np.float64)
    assert (ulps[~tie & ~saturated] >= MIN_GAP_ULPS).all()
    assert (np.diff(s.order)[tie | saturated] > 0).all()
    return int(tie.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_generators_and_restatement(name):
    case = make_case(name)
    ties = 0
    for b, s in enumerate(case.samples):
        ties += _check_sample(case, s)
        assert sort_path(s.M, case.A) == (case.path if len(case.samples) == 1 else
                                          (ONE_RUN, ONE_RUN, MERGED, IN_PLACE)[b])
        ref_b, ref_k, margin = reference(name)[b]
        exp = case.expected[b]
        assert len(exp) <= case.max_out and np.array_equal(ref_k, exp)
        if case.own is None and not hasattr(case, "nan_ids") and not name.startswith("equal"):
            assert len(exp) == min(s.M, case.max_out) and np.array_equal(exp, s.order[:case.max_out])
        if case.expected_classes is not None:
            pos = {int(a): i for i, a in enumerate(s.order)}
            assert np.array_equal(ref_b[:, 8], [case.expected_classes[b][pos[int(a)]] for a in ref_k])
        if case.nms == "rotated":
            assert margin >= 1e-6
    if name == "ties-classes":                         # the tie is between two classes of one anchor
        s = case.samples[0]
        assert ((s.cls[:, s.order].view(np.uint32) == s.logits.view(np.uint32)).sum(0)[::3] == 2).all()
    elif name.startswith("ties"):
        assert ties > 0
    if name == "ties-deep":
        assert ties == sum(hi - lo - 1 for lo, hi in TIE_GROUPS)
        order = case.samples[0].order                  # witnesses on both sides of every tie group's chunk / run edge
        for r in (255, 256, 16383, 16384, 32767, 32768, 65535, 65536, 131071, 131072):
            assert case.own_mask[order[r]]
    if name == "ties-top":
        assert (case.samples[0].logits[:600] == 20.0).all() and np.float32(1) / (np.float32(1) + np.exp(np.float32(-20))) == 1
    if name == "id-width":
        assert case.samples[0].order.max() == 2 ** 20 - 2 >= 2 ** 18 and case.samples[0].order.min() == 0
    if hasattr(case, "nan_ids"):
        assert not np.isin(case.nan_ids, ref_k).any() and len(ref_k) == 303
    if name == "deep-1":                               # both sides of every count at which the code changes path
        edges = (K_CHUNK, K_RUN, 2 * K_RUN, K_MAX_RUNS * K_RUN)
        assert {m for e in edges for m in (e, e + 1)} | {e - 1 for e in edges if e != 2 * K_RUN} <= set(BOUNDARY_PATHS)
        assert K_MAX_RUNS * K_RUN < A_BIG < 2 ** 18
    if name.startswith("deep") or name.startswith("pow2"):
        s = case.samples[0]
        want = [r for r in RANKS + (s.M - 2, s.M - 1) if 0 <= r < s.M]
        assert case.own_mask[s.order[want]].all()
        if s.M > 1000:
            assert len(case.expected[0]) >= 250          # the kept list is carried across every chunk


def test_too_many_anchors_are_refused_without_a_device():
    """A = 2^20 does not fit the key's 20-bit anchor-id field: PP_ERR_VALUE before any device work (the
    pointers are never followed)."""
    from pp_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    prm = _lib.DecodeParams(1024, 1024, 1, 1, 0.5, 0.1, 100, 0, 2048.0, 1.0, 1.0, 0.0, 0.0)
    rc = L.pp_decode_nms_batch_dev(fake, None, 1, fake, fake, 0, 1 << 20, 1, 0, 1 << 20, 1, fake, fake, fake, fake,
                                   ctypes.byref(prm), _lib.NMS_ANCHOR_RECT, 0, fake, fake, fake)
    assert rc == _lib.PP_ERR_VALUE and b"2^20" in L.pp_last_error()
    rc = L.pp_decode_dev(fake, None, fake, fake, fake, fake, fake, fake, ctypes.byref(prm), fake, fake, fake)
    assert rc == _lib.PP_ERR_VALUE and b"2^20" in L.pp_last_error()


# ---- the GPU part -----------------------------------------------------------------------------------

def _detector(gpu, case):
    from pp_amd.postprocess import Detector
    acfg = types.SimpleNamespace(fm_height=case.Hf, fm_width=case.Wf, per_cell=1)
    return Detector(case.anchors, acfg, *case.geometry, pos_thresh=case.pos_thresh, nms_thresh=case.nms_thresh,
                    max_out=case.max_out, num_classes=case.C, device=gpu, nms=case.nms, class_aware=case.class_aware)


def _check(boxes_d, kept_d, count_d, ref_b, ref_k, what):
    n = int(count_d.reshape(-1)[0].item())
    kept, got = kept_d.cpu().numpy(), boxes_d.cpu().numpy()
    if n != len(ref_k) or not np.array_equal(kept[:n], ref_k):
        m = min(n, len(ref_k))
        bad = np.nonzero(kept[:m] != ref_k[:m])[0]
        print(f"{what}: count {n}, expected {len(ref_k)}; first difference at {bad[:1]}\n got  {kept[:n].tolist()}"
              f"\n want {ref_k.tolist()}")
    assert n == len(ref_k), what
    assert np.array_equal(kept[:n], ref_k.astype(np.int32)), what
    assert (kept[n:] == -1).all(), what
    assert np.allclose(got[:n], ref_b, rtol=1e-5, atol=1e-5), what
    assert not got[n:].any(), what
    assert np.array_equal(got[:n, 8], ref_b[:, 8]), what


def _run(gpu, name):
    """The case through a Detector, twice (k_nms must re-arm the candidate counter on every path), each
    sample against the restatement and the closed form."""
    import torch
    case = make_case(name)
    ref = reference(name)
    det = _detector(gpu, case)
    B = len(case.samples)
    tc = torch.from_numpy(np.stack([case.cls_tensor(b) for b in range(B)])).to(gpu)
    tr = torch.from_numpy(np.stack([case.reg_tensor(b) for b in range(B)])).to(gpu)
    first = det(tc, tr)
    second = det(tc, tr)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.equal(x, y), name
    boxes_d, kept_d, count_d = second if B > 1 else (second[0][None], second[1][None], second[2])
    for b, s in enumerate(case.samples):
        ref_b, ref_k, margin = ref[b]
        if case.nms == "rotated":
            assert margin >= 1e-6
        assert np.array_equal(ref_k, case.expected[b])
        _check(boxes_d[b], kept_d[b], count_d.reshape(-1)[b:b + 1], ref_b, ref_k, f"{name}[{b}]")
    return case, det, tc, tr, second


@pytest.mark.gpu
@pytest.mark.parametrize("M", list(BOUNDARY_PATHS))
def test_path_boundaries_deep(gpu, M):
    """363 x 363 anchors, M candidates on both sides of every count at which the sort changes path."""
    case = _run(gpu, f"deep-{M}")[0]
    assert case.path == BOUNDARY_PATHS[M]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("shallow")])
def test_path_boundaries_shallow(gpu, name):
    case, _, _, _, (_, _, count) = _run(gpu, name)
    assert int(count.item()) == min(case.samples[0].M, case.max_out) == 1024


@pytest.mark.gpu
@pytest.mark.parametrize("A", list(POW2))
def test_power_of_two_anchor_counts(gpu, A):
    """cap == A == M: no run and no sort has any sentinel padding."""
    case = _run(gpu, f"pow2-{A}")[0]
    assert case.A == A == case.samples[0].M and case.path == POW2[A][1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["class-aware", "rotated"])
def test_in_place_sort_feeds_the_other_nms_forms(gpu, name):
    case = _run(gpu, name)[0]
    assert case.path == IN_PLACE and (case.class_aware or case.nms == "rotated")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ties-deep", "ties-deep-merged", "ties-top", "ties-classes"])
def test_score_ties(gpu, name):
    """Equal scores come out by ascending anchor id -- across chunk, run and merge boundaries -- and of two
    classes with the same maximal logit the lower is reported."""
    _run(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("nms", ["anchor", "rotated"])
def test_non_finite_class_logits(gpu, nms):
    """An anchor with a NaN score in any class is no candidate (torch.max propagates NaN); +inf is the score
    1.0, -inf the score 0.  A maximum that skips the NaN class (`if (s > score)` alone) keeps the six poisoned
    anchors that have a finite class above the threshold: 309 detections instead of 303."""
    case, _, _, _, (_, kept, count) = _run(gpu, f"nonfinite-{nms}")
    assert int(count.item()) == 303
    assert not np.isin(case.nan_ids, kept.cpu().numpy()).any()


@pytest.mark.gpu
def test_anchor_ids_use_all_twenty_bits(gpu):
    case, _, _, _, (_, kept, _) = _run(gpu, "id-width")
    assert int(kept.max().item()) == 2 ** 20 - 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["equal-at", "equal-below"])
def test_iou_equal_to_the_threshold(gpu, name):
    _run(gpu, name)


@pytest.mark.gpu
def test_mixed_batch(gpu):
    """No candidate, one run, merged runs and the in-place sort side by side in one call: every sample is
    bit-equal to its own call; then a smaller batch on the same scratch."""
    import torch
    case, det, tc, tr, (boxes_b, kept_b, count_b) = _run(gpu, "batch")
    assert [s.M for s in case.samples] == list(BATCH_M) and boxes_b.shape == (4, case.max_out, 9)
    assert int(count_b[0].item()) == 0
    for b in range(4):
        b1, k1, n1 = det(tc[b], tr[b])
        assert torch.equal(boxes_b[b], b1) and torch.equal(kept_b[b], k1) and count_b[b] == n1[0]
    b2, k2, n2 = det(tc[2:], tr[2:])
    assert torch.equal(b2, boxes_b[2:]) and torch.equal(k2, kept_b[2:]) and torch.equal(n2, count_b[2:])
