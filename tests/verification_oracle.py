"""Independent CPU restatement of the reference's verification metric (util/utils.py:370-395 perform_val's host math,
util/verification.py:38-87 calculate_roc, :224-234 calculate_accuracy): a pass over the pairs per threshold and fold, the way the
reference computes it, with sklearn's KFold and normalize.  Pinned to the reference by tests/golden/f21a_verification_metric.npz."""
import numpy as np
import sklearn.preprocessing
from sklearn.model_selection import KFold

THRESHOLDS = np.arange(0, 4, 0.01)


def _accuracy(threshold, dist, issame):
    pred = np.less(dist, threshold)
    tp = np.sum(np.logical_and(pred, issame))
    fp = np.sum(np.logical_and(pred, np.logical_not(issame)))
    tn = np.sum(np.logical_and(np.logical_not(pred), np.logical_not(issame)))
    fn = np.sum(np.logical_and(np.logical_not(pred), issame))
    tpr = 0 if (tp + fn == 0) else float(tp) / float(tp + fn)
    fpr = 0 if (fp + tn == 0) else float(fp) / float(fp + tn)
    return tpr, fpr, float(tp + tn) / dist.size


def roc_from_dist(dist, issame, n_folds=10, thresholds=THRESHOLDS):
    """-> (tpr, fpr, accuracy [n_folds], best_thresholds [n_folds])."""
    dist, issame = np.asarray(dist, np.float64), np.asarray(issame, bool)
    n_thr = len(thresholds)
    tprs, fprs = np.zeros((n_folds, n_thr)), np.zeros((n_folds, n_thr))
    accuracy, best = np.zeros(n_folds), np.zeros(n_folds)
    for f, (train, test) in enumerate(KFold(n_splits=n_folds, shuffle=False).split(np.arange(len(dist)))):
        acc_train = np.array([_accuracy(t, dist[train], issame[train])[2] for t in thresholds])
        k = int(np.argmax(acc_train))
        best[f] = thresholds[k]
        for j, t in enumerate(thresholds):
            tprs[f, j], fprs[f, j], _ = _accuracy(t, dist[test], issame[test])
        accuracy[f] = _accuracy(thresholds[k], dist[test], issame[test])[2]
    return np.mean(tprs, 0), np.mean(fprs, 0), accuracy, best


def embeddings_and_dist(emb_orig, emb_flip):
    """Per-copy embeddings [2P, D] each -> (normalised flip-summed embeddings, dist [P], xnorm) as perform_val computes them."""
    e0, e1 = np.asarray(emb_orig, np.float64), np.asarray(emb_flip, np.float64)
    xnorm, cnt = 0.0, 0
    for e in (e0, e1):
        for row in e:
            xnorm += np.linalg.norm(row)
            cnt += 1
    emb = sklearn.preprocessing.normalize(e0 + e1)
    dist = np.sum(np.square(np.subtract(emb[0::2], emb[1::2])), 1)
    return emb, dist, xnorm / cnt


def perform_val(emb_orig, emb_flip, issame, n_folds=10):
    """-> (acc_mean, acc_std, xnorm, best_threshold_mean, tpr, fpr, accuracy, best_thresholds)."""
    _, dist, xnorm = embeddings_and_dist(emb_orig, emb_flip)
    tpr, fpr, accuracy, best = roc_from_dist(dist, issame, n_folds)
    return accuracy.mean(), accuracy.std(), xnorm, best.mean(), tpr, fpr, accuracy, best
