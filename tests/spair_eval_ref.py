"""numpy restatements of the SPAIR evaluation kernels (spair_eval.hip): tf.image.draw_bounding_boxes (TF 2.0's
DrawBoundingBoxesOp, as spair/visualizer.py:107-111 calls it) and the count metrics of spair/trainer.py:294-301.
TensorFlow cannot run here: these restatements are the pin the kernels are tested against."""
import numpy as np

INT64_MIN = np.iinfo(np.int64).min


def tf_trunc_i64(v):
    """(int64)(fp32 v): toward zero; NaN or beyond the int64 range -> INT64_MIN (x86's cvttss2si, where TF runs the op)."""
    v = np.float32(v)
    if not (v >= np.float32(-2.0 ** 63) and v < np.float32(2.0 ** 63)):
        return INT64_MIN
    return int(np.trunc(np.float64(v)))


def box_rows_cols(box, H, W):
    """(r0, c0, r1, c1) of one (ymin, xmin, ymax, xmax) box, computed in fp32 as TF does."""
    ymin, xmin, ymax, xmax = (np.float32(v) for v in box)
    fh, fw = np.float32(H - 1), np.float32(W - 1)
    return (tf_trunc_i64(ymin * fh), tf_trunc_i64(xmin * fw), tf_trunc_i64(ymax * fh), tf_trunc_i64(xmax * fw))


def draw_bounding_boxes(images, boxes, colors, gate=None):
    """images [B,H,W,C] fp32, boxes [B,NB,4], colors [NC,ldc] (ldc >= C), gate [B,NB] or None -> a new [B,H,W,C] array."""
    out = np.array(images, dtype=np.float32, copy=True)
    B, H, W, C = out.shape
    boxes = np.asarray(boxes, dtype=np.float32)
    colors = np.asarray(colors, dtype=np.float32)
    if gate is not None:
        boxes = boxes * np.asarray(gate, dtype=np.float32).reshape(B, -1, 1)       # obj_bbox_mask * z_pres (fp32)
    for b in range(B):
        for bb in range(boxes.shape[1]):
            col = colors[bb % colors.shape[0], :C]
            r0, c0, r1, c1 = box_rows_cols(boxes[b, bb], H, W)
            if r0 > r1 or c0 > c1:                                                  # inverted
                continue
            if r0 >= H or r1 < 0 or c0 >= W or c1 < 0:                              # completely outside
                continue
            r0c, r1c, c0c, c1c = max(r0, 0), min(r1, H - 1), max(c0, 0), min(c1, W - 1)
            if r0 >= 0:
                out[b, r0, c0c:c1c + 1, :] = col
            if r1 < H:
                out[b, r1, c0c:c1c + 1, :] = col
            if c0 >= 0:
                out[b, r0c:r1c + 1, c0, :] = col
            if c1 < W:
                out[b, r0c:r1c + 1, c1, :] = col
    return out


def sigmoid32(x):
    x = np.asarray(x, dtype=np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def count_metrics(z_pres_logits, labels):
    """-> (pred [B] fp32, MAE, MAPE, matches) of spair/trainer.py:294-301: pred = sum of round-half-even(sigmoid) over the cells,
    Keras mean_absolute_error / mean_absolute_percentage_error (epsilon 1e-7) and tf.keras.metrics.Accuracy's match count."""
    lg = np.asarray(z_pres_logits, dtype=np.float32)
    B = lg.shape[0]
    lg = lg.reshape(B, -1)
    pred = np.zeros((B,), np.float32)
    for c in range(lg.shape[1]):                                                    # cell order
        pred += np.rint(sigmoid32(lg[:, c]))
    lab = np.asarray(labels, dtype=np.float32).reshape(B)
    d = np.abs(lab.astype(np.float64) - pred)
    mae = float(d.mean())
    mape = float(100.0 * (d / np.maximum(np.abs(lab.astype(np.float64)), 1e-7)).mean())
    return pred, mae, mape, int((pred == lab).sum())
