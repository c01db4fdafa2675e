"""float64 NumPy twin of sv_knn_classify (include/splitvae.h): row norms, d = max(0, n(q) + n(r) - 2 q.r), the neighbours under the
total order (d, reference index), the vote with ties to the lowest class id."""
import numpy as np


def norms(v):
    v = np.asarray(v, np.float64)
    return (v * v).sum(axis=1)


def distances(q, r):
    """[Nq, Nr] float64: the expansion formula of the header, clamped at 0."""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    return np.maximum(0.0, (norms(q)[:, None] + norms(r)[None, :]) - 2.0 * (q @ r.T))


def neighbours(d, k):
    """(index [Nq,k] int32, dist [Nq,k] float64): per row the k smallest under (d, index), ascending.  A stable argsort of the
    distances IS that order: equal distances keep their index order."""
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(d, order, axis=1)


def vote(nn_index, r_class, n_class):
    """pred [Nq] int32: the class with the most votes among the neighbours; np.argmax returns the first, i.e. lowest, class of a tie."""
    cls = np.asarray(r_class)[nn_index]
    counts = np.stack([(cls == c).sum(axis=1) for c in range(n_class)], axis=1)
    return counts.argmax(axis=1).astype(np.int32)


def classify(q, r, r_class, k, n_class):
    """-> (nn_index, nn_dist, pred, d): the twin of one sv_knn_classify call; d is the full distance matrix."""
    d = distances(q, r)
    idx, dist = neighbours(d, k)
    return idx, dist, vote(idx, r_class, n_class), d


def boundary_gap(d, k):
    """Per query the float64 relative gap (d_(k+1) - d_(k)) / d_(k+1) between the k-th and the (k+1)-th smallest distance: how
    far the neighbour SET is from changing.  +inf when there is no (k+1)-th reference; 0 for an exact tie (also at d = 0)."""
    d = np.asarray(d, np.float64)
    if d.shape[1] <= k:
        return np.full(d.shape[0], np.inf)
    s = np.sort(d, axis=1)
    dk, dk1 = s[:, k - 1], s[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(dk1 > 0, (dk1 - dk) / dk1, 0.0)
