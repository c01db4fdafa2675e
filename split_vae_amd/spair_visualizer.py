"""The figures of spair/visualizer.py and the in-loop canvas of spair/trainer.py:331-378 for SPAIR / SPLIT-SPAIR.

Same function names, signatures and file names as the reference (its spelling "reconstrcution" included).  The reference renders
each canvas through matplotlib; here the canvas itself is written as an 8-bit RGB PNG by visualizer.save_png, and a figure of
several subplots puts its panels side by side in subplot order with a 4-pixel white gutter between them.  The boxes of
reconstruction_bbox are drawn on the device by sv_draw_bounding_boxes (tf.image.draw_bounding_boxes).

Deviations from the reference:
- the first test batch is used, not test_dataset.take(n).shuffle(n, seed=1);
- the training canvas slices the actual batch where spair/trainer.py:346-347 hard-codes a batch of 32;
- no titles, ticks, grid lines or colormaps (a one-channel canvas is written grey);
- glimpses_local_reconstruction_test is not ported: it serves 'lg_glimpse_spair', whose model class is undefined upstream.
Every function also takes `outputs`: the model's returned tuple for the first n test images, computed when not given.
"""
import os

import numpy as np
import torch

from . import ops
from .visualizer import _first_batch, _np, save_png

GUTTER = 4
WHITE = [[1.0, 1.0, 1.0, 1.0]]          # spair/visualizer.py:108


def _side_by_side(panels):
    """Panels [h, w_i, 3] in subplot order -> one canvas, a GUTTER-pixel white column between neighbours."""
    h = panels[0].shape[0]
    gap = np.ones((h, GUTTER, 3), np.float32)
    parts = []
    for i, p in enumerate(panels):
        if i:
            parts.append(gap)
        parts.append(p)
    return np.concatenate(parts, axis=1)


def _rgb(canvas):
    """[h, w] or [h, w, 1] grey -> [h, w, 3]; [h, w, 3] unchanged."""
    c = np.asarray(canvas, np.float32)
    if c.ndim == 2:
        c = c[..., None]
    return np.repeat(c, 3, axis=2) if c.shape[2] == 1 else c


def _strip(x, n):
    """x [>= n, h, w, c] -> [h, n*w, c]: image i in columns [i*w, (i+1)*w)."""
    x = x[:n]
    return np.concatenate(list(x), axis=1)


def _cells(x, n):
    """x [>= n, cells, h, w, c] -> [cells*h, n*w, c]: column block i = image i's cells stacked (reshape((cells*h, w, c)))."""
    x = x[:n]
    return np.concatenate([xi.reshape((-1,) + xi.shape[2:]) for xi in x], axis=1)


def _out(filepath, name):
    return os.path.join(filepath or "", name + ".png")


def recon_panels(images, x_recon, z_pres, z_depth, obj_full_recon_unnorm, n):
    """The three canvases of spair/visualizer.py:14-81 (and spair/trainer.py:331-378), each [(cells+2)*H, n*W, 3]: rows 0-1 the
    input and x_recon, then one row per cell of obj_recon (panel 1), obj_recon * alpha * z_pres * sigmoid(-z_depth) (panel 2) and
    z_pres in channel 0 (panel 3: channels 1-2 are zero here; upstream they are np.empty, whatever memory held)."""
    img = _np(images[:n])
    C = min(3, img.shape[3])
    full = _np(obj_full_recon_unnorm[:n])                     # [n, cells, H, W, C+1]
    cells = full.shape[1]
    obj_recon, obj_alpha = full[..., :C], full[..., C:C + 1]
    zp = _np(z_pres[:n]).reshape(n, cells, 1, 1, 1)
    zd = _np(z_depth[:n]).reshape(n, cells, 1, 1, 1)
    head = np.concatenate([_strip(img[..., :C], n), _strip(_np(x_recon[:n])[..., :C], n)], axis=0)
    sig = (1.0 / (1.0 + np.exp(zd.astype(np.float32)))).astype(np.float32)     # sigmoid(-z_depth)
    weighted = obj_recon * obj_alpha * zp * sig
    pres = np.zeros(obj_recon.shape, np.float32)
    pres[..., 0] = np.broadcast_to(zp[..., 0], obj_recon.shape[:-1])
    return [_rgb(np.concatenate([head, _cells(body, n)], axis=0)) for body in (obj_recon, weighted, pres)]


def train_reconstruction(images, step_outputs, step=0, filepath=None, n=10):
    """spair/trainer.py:331-378: train_recon_it_<step>.png from the train step's own outputs (its sampled z_pres).  step_outputs: the
    tuple train_step returns (x_recon, ..., z_depth at 7, z_pres at 10, ..., obj_full_recon_unnorm at 16, ...).  Returns the canvas."""
    n = min(n, int(images.shape[0]))
    panels = recon_panels(images, step_outputs[0], step_outputs[10], step_outputs[7], step_outputs[16], n)
    canvas = _side_by_side(panels)
    save_png(_out(filepath, "train_recon_it_" + str(step)), canvas)
    return canvas


def _eval(model, test_dataset, label, n, outputs):
    images = _first_batch(test_dataset, label)
    n = min(n, int(images.shape[0]))
    x_test = images[:n].contiguous()
    if outputs is None:
        with torch.no_grad():
            outputs = model(x_test)                               # model(x_test): training=False
    return x_test, n, outputs


def _rounded_pres(z_pres_logits):
    return torch.round(torch.sigmoid(z_pres_logits))              # tf.round(tf.sigmoid(z_pres_logits)) (:36, :103)


def reconstruction_test(model, test_dataset, filename=None, filepath=None, label=True, n=10, outputs=None):
    """spair/visualizer.py:14-81: x_reconstrcution_test{filename}.png, the layout of recon_panels with z_pres = round(sigmoid(logits))."""
    x_test, n, o = _eval(model, test_dataset, label, n, outputs)
    panels = recon_panels(x_test, o[0], _rounded_pres(o[11]), o[7], o[16], n)
    canvas = _side_by_side(panels)
    save_png(_out(filepath, "x_reconstrcution_test" + filename if filename is not None else "x_reconstrcution_test_spair"), canvas)
    return canvas


def reconstruction_bbox(model, test_dataset, filename=None, filepath=None, label=True, n=10, outputs=None):
    """spair/visualizer.py:84-137: x_reconstrcution_bbox{filename}.png, rows = input | input with boxes | x_recon with boxes, each
    [H, n*W, 3]; the boxes are obj_bbox_mask * round(sigmoid(z_pres_logits)) in one white colour (sv_draw_bounding_boxes)."""
    x_test, n, o = _eval(model, test_dataset, label, n, outputs)
    x3 = x_test[..., :3].contiguous()
    bbox = o[17].contiguous()
    gate = _rounded_pres(o[11]).reshape(n, -1).contiguous()
    colors = torch.tensor(WHITE, dtype=torch.float32, device=x3.device)
    img_w_bbox = ops.draw_bounding_boxes(x3, bbox, colors, gate=gate)
    x_recon_w_bbox = ops.draw_bounding_boxes(o[0][..., :3].contiguous(), bbox, colors, gate=gate)
    canvas = _rgb(np.concatenate([_strip(_np(x3), n), _strip(_np(img_w_bbox), n), _strip(_np(x_recon_w_bbox), n)], axis=0))
    save_png(_out(filepath, "x_reconstrcution_bbox" + filename if filename is not None else "x_reconstrcution_bbox"), canvas)
    return canvas


def glimpses_reconstruction_test(model, test_dataset, filename=None, filepath=None, label=True, n=10, outputs=None):
    """spair/visualizer.py:140-202: glimpses{filename}.png, three panels of [cells*S, n*S, 3] (S = object_size): all_glimpses,
    obj_recon_unnorm and obj_recon_alpha (grey)."""
    x_test, n, o = _eval(model, test_dataset, label, n, outputs)
    C = min(3, int(x_test.shape[3]))
    panels = [_rgb(_cells(_np(o[13])[..., :C], n)), _rgb(_cells(_np(o[14])[..., :C], n)), _rgb(_cells(_np(o[15]), n))]
    canvas = _side_by_side(panels)
    save_png(_out(filepath, "glimpses" + filename if filename is not None else "glimpses"), canvas)
    return canvas


def x_hat_reconstruction_test(model, test_dataset, filename=None, filepath=None, label=True, n=10, outputs=None):
    """spair/visualizer.py:259-285 (lg_spair): x_hat_reconstrcution_test{filename}.png, x_hat_recon over the x_hat input, [2H, n*W, 3]."""
    x_test, n, o = _eval(model, test_dataset, label, n, outputs)
    canvas = _rgb(np.concatenate([_strip(_np(o[21])[..., :3], n), _strip(_np(x_test)[..., 3:6], n)], axis=0))
    save_png(_out(filepath, "x_hat_reconstrcution_test" + filename if filename is not None else "x_hat_reconstrcution_test_lg_vae"),
             canvas)
    return canvas


def write_test_figures(model, test_ds, config, step, test_num, filepath):
    """The figures spair/trainer.py:403-414 writes after test set `test_num` at a log step."""
    tag = "_it_" + str(step) + "_" + str(test_num)
    label = isinstance(next(iter(test_ds)), (tuple, list))       # (images, labels) batches, as the loop reads them
    reconstruction_test(model, test_ds, filename=tag, filepath=filepath, label=label)
    reconstruction_bbox(model, test_ds, filename=tag, filepath=filepath, label=label)
    glimpses_reconstruction_test(model, test_ds, filename=tag, filepath=filepath, label=label)
    if config.model == "lg_spair":
        x_hat_reconstruction_test(model, test_ds, filename=tag, filepath=filepath, label=label)
