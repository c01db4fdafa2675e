"""NumPy twin of the detection average precision, written from the definitions, not from csrc/detect_ap.hip:
the IoU test in np.float32 with one rounding per operation, the matching as plain Python loops, the curve in float64 through an
argsort on (-logit, id), a cumulative sum and a reversed running maximum.  `mutant` names one deliberate mistake (MUTANTS): the
tests check that the comparison against the library rejects every one of them on the inputs it accepts the twin on.  The case
generators the host and the GPU tests share live here too."""
import struct

import numpy as np

F = np.float32
NONDET = 0xFFFFFFFF
MUTANTS = ("strict_threshold", "tie_high_box", "reuse_boxes", "extent_plus_one", "ascending", "sigmoid_keys", "no_interpolation",
           "g_from_count")


# ---------------------------------------------------------------------------------------------- extents and ground truth
def sprite_extents(bank):
    """int32 [n,4] inclusive (r0, c0, r1, c1) of the pixels with max(r,g,b) > 0; -1 four times for an empty sprite."""
    out = np.full((len(bank), 4), -1, np.int32)
    for s, sp in enumerate(np.asarray(bank)):
        on = sp.max(axis=-1) > 0
        if on.any():
            rows, cols = np.nonzero(on.any(axis=1))[0], np.nonzero(on.any(axis=0))[0]
            out[s] = (rows[0], cols[0], rows[-1], cols[-1])
    return out


def gt_boxes(layouts, extents, mutant=None):
    """(boxes [B,5,4] float32, n_gt [B] int32) of structured layouts (count, row, col, sprite)."""
    B = len(layouts)
    boxes, n_gt = np.zeros((B, 5, 4), F), np.zeros((B,), np.int32)
    one = 0 if mutant == "extent_plus_one" else 1
    for b, L in enumerate(layouts):
        n = 0
        for k in range(min(max(int(L["count"]), 0), 5)):
            s = int(L["sprite"][k])
            if not 0 <= s < len(extents) or extents[s][0] < 0:
                continue
            r0, c0, r1, c1 = (int(v) for v in extents[s])
            row, col = int(L["row"][k]), int(L["col"][k])
            boxes[b, n] = (F(row + r0) / F(48), F(col + c0) / F(48), F(row + r1 + one) / F(48), F(col + c1 + one) / F(48))
            n += 1
        n_gt[b] = n
    return boxes, n_gt


# ---------------------------------------------------------------------------------------------- matching
def _is_area(b):
    return bool(np.all(np.isfinite(b)) and b[2] > b[0] and b[3] > b[1])


def iou_terms(d, g):
    """(inter, union, iou) in float32, one rounding per operation; (0, 0, 0) unless both are areas that intersect."""
    d, g = np.asarray(d, F), np.asarray(g, F)
    if not (_is_area(d) and _is_area(g)):
        return F(0), F(0), F(0)
    ih = F(min(d[2], g[2]) - max(d[0], g[0]))
    iw = F(min(d[3], g[3]) - max(d[1], g[1]))
    if not (ih > 0 and iw > 0):
        return F(0), F(0), F(0)
    inter = F(ih * iw)
    a = F(F(d[2] - d[0]) * F(d[3] - d[1]))
    b = F(F(g[2] - g[0]) * F(g[3] - g[1]))
    union = F(F(a + b) - inter)
    if not inter > 0:
        return F(0), F(0), F(0)
    return inter, union, F(inter / union)


def passes(inter, union, t, mutant=None):
    if not inter > 0:
        return False
    lhs, rhs = F(F(10) * inter), F(F(t) * union)
    return bool(lhs > rhs) if mutant == "strict_threshold" else bool(lhs >= rhs)


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _sigmoid32(v):
    with np.errstate(over="ignore"):
        return F(F(1) / F(F(1) + np.exp(-F(v), dtype=F)))


def record_key(logit, ident, mutant=None):
    """Ascending key order = descending logit, then ascending id; a non-detection sorts last."""
    logit = F(logit)
    if not logit > 0:
        return (NONDET << 32) | ident
    conf = _sigmoid32(logit) if mutant == "sigmoid_keys" else logit
    u = _bits(conf)                                  # positive floats: the bit pattern grows with the value
    hi = u if mutant == "ascending" else 0x7FFFFFFF - u
    return (hi << 32) | ident


def match(bbox, logits, gt, n_gt, image_offset=0, mutant=None):
    """bbox [B,cells,4], logits [B,cells], gt [B,5,4], n_gt [B] -> (keys uint64 [B*cells], tp uint16 [B*cells]) of the B images."""
    bbox, logits, gt = np.asarray(bbox, F), np.asarray(logits, F), np.asarray(gt, F)
    B, cells = logits.shape
    keys, tps = np.zeros((B * cells,), np.uint64), np.zeros((B * cells,), np.uint16)
    for b in range(B):
        ng = min(max(int(n_gt[b]), 0), 5)
        ids = [(image_offset + b) * cells + j for j in range(cells)]
        k = [record_key(logits[b, j], ids[j], mutant) for j in range(cells)]
        dets = sorted((j for j in range(cells) if logits[b, j] > 0), key=lambda j: k[j])
        terms = {(j, g): iou_terms(bbox[b, j], gt[b, g]) for j in dets for g in range(ng)}
        mask = [0] * cells
        for t in range(1, 10):
            taken = set()
            for j in dets:
                best, best_iou = None, None
                for g in range(ng):
                    inter, union, iou = terms[(j, g)]
                    if (g in taken and mutant != "reuse_boxes") or not passes(inter, union, t, mutant):
                        continue
                    better = best is None or iou > best_iou or (mutant == "tie_high_box" and iou == best_iou)
                    if better:
                        best, best_iou = g, iou
                if best is not None:
                    taken.add(best)
                    mask[j] |= 1 << (t - 1)
        for j in range(cells):
            keys[b * cells + j] = k[j]
            tps[b * cells + j] = mask[j]
    return keys, tps


# ---------------------------------------------------------------------------------------------- the curve
def key_logits(keys):
    """(is_detection bool, logit float32, id int64) decoded from record keys."""
    keys = np.asarray(keys, np.uint64)
    hi, ident = (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    det = hi != NONDET
    u = (np.uint32(0x7FFFFFFF) - np.where(det, hi, 0).astype(np.uint32)).astype(np.uint32)
    return det, u.view(np.float32), ident


def curve(keys, tps, G, mutant=None):
    """dict(ap [9], ap_un [9] float64, tp [9], M, G) of records in any order."""
    det, logit, ident = key_logits(keys)
    tps = np.asarray(tps).astype(np.int64)[det]
    logit, ident = logit[det].astype(np.float64), ident[det]
    order = np.lexsort((ident, -logit))              # primary: descending logit; ties: the lower id
    tps = tps[order]
    M, G = int(det.sum()), int(G)
    ap, ap_un, tot = np.zeros(9), np.zeros(9), np.zeros(9, np.int64)
    for t in range(9):
        hit = (tps >> t) & 1
        tot[t] = hit.sum()
        if M == 0 or G == 0:
            continue
        p = np.cumsum(hit).astype(np.float64) / np.arange(1, M + 1, dtype=np.float64)
        envelope = np.maximum.accumulate(p[::-1])[::-1]
        ap_un[t] = (p * hit).sum() / G
        ap[t] = ap_un[t] if mutant == "no_interpolation" else (envelope * hit).sum() / G
    return dict(ap=ap, ap_un=ap_un, tp=tot, M=M, G=G)


def evaluate(bbox, logits, gt, n_gt, counts=None, mutant=None):
    """The whole report of one test set: match + curve.  counts: the layouts' object counts (what the g_from_count mutant sums)."""
    keys, tps = match(bbox, logits, gt, n_gt, 0, mutant)
    G = int(np.sum(counts)) if mutant == "g_from_count" else int(np.clip(np.asarray(n_gt), 0, 5).sum())
    res = curve(keys, tps, G, mutant)
    M = res["M"]
    res.update(mAP=float(res["ap"].mean()), ap50=float(res["ap"][4]), precision50=(res["tp"][4] / M if M else 0.0),
               recall50=(res["tp"][4] / G if G else 0.0))
    return res


# ---------------------------------------------------------------------------------------------- shared cases
LOGIT_POOL = np.array([-np.inf, -1.0, -0.0, 0.0, np.nan, 0.5, 0.5, 1.0, 2.0, 2.0, 20.0, 30.0, np.inf, 1e-40], F)


def _lattice_box(rng):
    y0, x0 = rng.integers(-8, 64, 2)
    h, w = rng.integers(-4, 40, 2)                   # h or w <= 0: inverted or zero-area boxes
    return np.array([y0, x0, y0 + h, x0 + w], np.float64) / 64.0


def lattice_case(cells, B=12, seed=0):
    """Boxes on the 1/64 lattice (every area, intersection and union is exact in fp32, so exact ties with a threshold are decided the
    same way everywhere), logits from a pool with exact ties, +-0, NaN and +-inf.  The first images are hand-built: an exact tie
    IoU == t/10 for every t, identical / nested / touching / inverted / zero-area boxes, the symmetric tie between two boxes, a
    duplicate detection, and a detection whose best box is taken while its second-best passes."""
    rng = np.random.default_rng([seed, cells, 0xDA])
    bbox, logits = np.zeros((B, cells, 4), F), np.full((B, cells), -1.0, F)
    gt, n_gt = np.zeros((B, 5, 4), F), np.zeros((B,), np.int32)
    for b in range(B):
        n_gt[b] = b % 6
        for g in range(5):
            gt[b, g] = _lattice_box(rng)
            if g < n_gt[b] and rng.random() < 0.8:   # mostly real areas among the boxes that count
                gt[b, g, 2:] = gt[b, g, :2] + rng.integers(4, 30, 2) / 64.0
        for j in range(cells):
            bbox[b, j] = _lattice_box(rng) if rng.random() < 0.5 or n_gt[b] == 0 else gt[b, rng.integers(n_gt[b])] + rng.integers(-3, 4, 4) / 64.0
            logits[b, j] = LOGIT_POOL[rng.integers(len(LOGIT_POOL))]
    u = 1.0 / 64.0

    def put(b, boxes, dets):
        n_gt[b] = len(boxes)
        gt[b] = 0
        gt[b, :len(boxes)] = np.asarray(boxes, np.float64) * u
        logits[b] = -1.0
        for j, (box, lg) in enumerate(dets[:cells]):
            bbox[b, j], logits[b, j] = np.asarray(box, np.float64) * u, lg

    # image 0: box 10 x 10, detections 10 x t nested in it: IoU == t / 10 exactly; plus identical, touching, inverted, zero-area
    put(0, [(0, 0, 10, 10), (20, 20, 30, 30)],
        [((0, 0, 10, t), 10.0 - t) for t in range(1, 10)] + [((20, 20, 30, 30), 0.25), ((30, 20, 40, 30), 0.2), ((30, 30, 20, 20), 0.15),
                                                             ((20, 20, 20, 30), 0.1), ((0, 0, 10, 10), 0.05)])
    # image 1: A sits symmetrically between two boxes (equal IoU: takes box 0), B overlaps box 0 only -> false positive
    put(1, [(0, 0, 8, 8), (0, 8, 8, 16)], [((0, 4, 8, 12), 3.0), ((0, 0, 8, 6), 2.0)])
    # image 2: a duplicate detection of one box; image 3: the best box is taken, the second-best passes
    put(2, [(0, 0, 8, 8)], [((0, 0, 8, 8), 2.0), ((0, 0, 8, 8), 2.0), ((0, 0, 8, 7), 1.0)])
    put(3, [(0, 0, 8, 8), (0, 4, 8, 12)], [((0, 0, 8, 8), 3.0), ((0, 1, 8, 9), 2.0)])
    # image 4: saturating logits in id order 20, 30 (equal sigmoids in fp32), only the second is a true positive
    put(4, [(0, 0, 8, 8)], [((40, 40, 48, 48), 20.0), ((0, 0, 8, 8), 30.0)])
    return dict(bbox=bbox, logits=logits, gt=gt, n_gt=n_gt)


def _iou64(d, g):
    if not (d[2] > d[0] and d[3] > d[1] and g[2] > g[0] and g[3] > g[1]):
        return 0.0
    ih, iw = min(d[2], g[2]) - max(d[0], g[0]), min(d[3], g[3]) - max(d[1], g[1])
    if ih <= 0 or iw <= 0:
        return 0.0
    inter = ih * iw
    return inter / ((d[2] - d[0]) * (d[3] - d[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter)


def random_case(cells, B=24, seed=0):
    """Seeded float boxes over [-0.3, 1.3]; an image in which a float64 IoU lies within 1e-5 of a threshold is redrawn, so no pair is
    excluded at comparison time.  -> (case, redraws)."""
    rng = np.random.default_rng([seed, cells, 0xDB])
    bbox, logits = np.zeros((B, cells, 4), F), np.zeros((B, cells), F)
    gt, n_gt = np.zeros((B, 5, 4), F), np.zeros((B,), np.int32)
    redraws = 0
    for b in range(B):
        while True:
            ng = int(rng.integers(0, 6))
            g = np.sort(rng.uniform(-0.3, 1.3, (5, 2, 2)), axis=1).transpose(0, 2, 1).reshape(5, 4)[:, [0, 2, 1, 3]].astype(F)
            d = rng.uniform(-0.3, 1.3, (cells, 4)).astype(F)
            near = rng.random(cells) < 0.5
            d = np.where(near[:, None], g[rng.integers(0, 5, cells)] + rng.normal(0, 0.04, (cells, 4)).astype(F), d).astype(F)
            ious = [_iou64(d[j].astype(np.float64), g[q].astype(np.float64)) for j in range(cells) for q in range(ng)]
            if any(abs(v - t / 10.0) < 1e-5 for v in ious for t in range(1, 10)):
                redraws += 1
                continue
            break
        bbox[b], gt[b], n_gt[b] = d, g, ng
        logits[b] = rng.normal(0.3, 2.0, cells).astype(F)
    return dict(bbox=bbox, logits=logits, gt=gt, n_gt=n_gt), redraws


def random_records(n, seed=0, kind="random"):
    """(keys uint64 [n], tps uint16 [n], G): records for the finish call.  kind: random (many non-detections), all_tp, all_fp,
    sorted, reversed."""
    rng = np.random.default_rng([seed, n, 0xDC])
    logits = rng.normal(0.0, 2.0, n).astype(F)
    if kind != "random":
        logits = np.abs(logits) + F(1e-3)
    logits[rng.random(n) < 0.1] = F(1.5)              # exact ties: decided by the id
    ids = rng.permutation(n) if kind in ("random", "all_tp", "all_fp") else np.arange(n)
    hi = np.where(logits > 0, np.uint32(0x7FFFFFFF) - logits.view(np.uint32), np.uint32(NONDET)).astype(np.uint64)
    keys = (hi << np.uint64(32)) | ids.astype(np.uint64)
    assert all(int(keys[i]) == record_key(logits[i], int(ids[i])) for i in range(min(n, 64)))
    tps = rng.integers(0, 512, n).astype(np.uint16)
    tps = np.where(rng.random(n) < 0.4, 0, tps).astype(np.uint16)
    if kind == "all_tp":
        tps[:] = 511
    if kind == "all_fp":
        tps[:] = 0
    if kind in ("sorted", "reversed"):
        order = np.argsort(keys)
        order = order[::-1] if kind == "reversed" else order
        keys, tps = keys[order], tps[order]
    tps[(keys >> np.uint64(32)) == NONDET] = 0
    G = int(max(1, (tps != 0).sum() + n // 7))
    return keys, tps, G
