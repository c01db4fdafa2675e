"""Detection average precision of SPAIR / SPLIT-SPAIR on the Multi-Bird test canvases (--detection_ap).

No reference counterpart: spair/data.py throws away the positions it pastes the birds at, so the reference reports the count
accuracy only.  Here canvas i of a split is a pure function of (seed, split, i) (csrc/multibird.hip), so its ground-truth boxes
are too: the layout's positions plus the tight extents of the sprites' masks (`ground_truth`).  A detection is a cell with
z_pres_logits > 0 -- the cells the count metric counts --, its box the cell's obj_bbox_mask row, its confidence the logit.
DESIGN.md section 4.20 pins the matching and the curve; csrc/detect_ap.hip computes both on the device: one launch per batch
(sv_detect_match) beside the count metrics, one finish call and one read-back per test set.  This is the project's own definition
of AP@IoU; it is not pinned against the original SPAIR evaluation code.
"""
import torch

from . import ops

THRESHOLDS = tuple(t / 10.0 for t in range(1, 10))
UNAVAILABLE = 'Note: --detection_ap needs the ground-truth boxes of kernel-rendered Multi-Bird canvases; skipped'
REPORT = ('Detection AP{}: mean {:.4f} (IoU 0.1 .. 0.9), AP@0.5 {:.4f}, precision@0.5 {:.4f}, recall@0.5 {:.4f} '
          '({} detections, {} boxes)')


def ground_truth(bank, bg, n_sprites, n, seed, split):
    """(boxes [n,5,4] fp32, n_boxes [n] int32) of canvases 0 .. n-1 of `split`, on the bank's device: two launches."""
    layouts = ops.multibird_layouts(n, bg, n_sprites, seed, split, device=bank.device)
    return ops.multibird_gt_boxes(layouts, ops.sprite_extents(bank))


class DetectionAP:
    """The records of one test set (n_images images of `cells` cells) and the workspace of the finish call.  update() appends a
    batch at a host-known image offset; result() is one sv_detect_ap_finish and one read-back.  Same life cycle as CountAccuracy."""

    def __init__(self, device, n_images, cells):
        n_images, cells = int(n_images), int(cells)
        if n_images < 1 or not 1 <= cells <= ops.DETECT_AP_MAX_CELLS or n_images * cells > ops.DETECT_AP_MAX_RECORDS:
            raise ValueError("DetectionAP: %d images of %d cells (1 .. %d cells, at most %d records)"
                             % (n_images, cells, ops.DETECT_AP_MAX_CELLS, ops.DETECT_AP_MAX_RECORDS))
        self.n_images, self.cells = n_images, cells
        n = n_images * cells
        self.rec_key = torch.empty((n,), dtype=torch.int64, device=device)
        self.rec_tp = torch.empty((n,), dtype=torch.int16, device=device)
        self.n_gt = torch.zeros((n_images,), dtype=torch.int32, device=device)
        self.workspace = torch.empty((ops.detect_ap_workspace_bytes(n),), dtype=torch.uint8, device=device)
        self.out = torch.empty((ops.DETECT_AP_OUT,), dtype=torch.float64, device=device)
        self.seen = 0

    def update(self, bbox, logits, gt_boxes, n_gt):
        """bbox [B,cells,4], logits [B,cells,...] of the next B images, their gt_boxes [B,5,4] and n_gt [B] (int32)."""
        B = int(bbox.shape[0])
        if self.seen + B > self.n_images:
            raise ValueError("DetectionAP.update: %d images beyond the %d it was made for" % (self.seen + B, self.n_images))
        if logits.numel() != B * self.cells:
            raise ValueError("DetectionAP.update: %d logits for %d images of %d cells" % (logits.numel(), B, self.cells))
        ops.detect_match(bbox, logits, gt_boxes, n_gt, self.rec_key, self.rec_tp, image_offset=self.seen)
        self.n_gt[self.seen:self.seen + B].copy_(n_gt.reshape(-1))
        self.seen += B

    def result(self):
        """dict(mAP, ap [9], ap_uninterpolated [9], ap50, precision50, recall50, tp [9], detections, boxes, images) over the images
        seen so far; None before the first update."""
        if not self.seen:
            return None
        ops.detect_ap_finish(self.rec_key, self.rec_tp, self.n_gt[:self.seen], n_records=self.seen * self.cells,
                             workspace=self.workspace, out=self.out)
        host = self.out.cpu()
        ap, apu = host[:9].tolist(), host[9:18].tolist()
        ints = host.view(torch.int64)[18:].tolist()
        tp, M, G = ints[:9], ints[9], ints[10]
        return dict(mAP=sum(ap) / 9.0, ap=ap, ap_uninterpolated=apu, ap50=ap[4], precision50=(tp[4] / M if M else 0.0),
                    recall50=(tp[4] / G if G else 0.0), tp=tp, detections=M, boxes=G, images=self.seen)

    def reset_states(self):
        self.seen = 0
        self.n_gt.zero_()


def report_line(res, test_num):
    return REPORT.format(test_num, res["mAP"], res["ap50"], res["precision50"], res["recall50"], res["detections"], res["boxes"])


def history_entries(res, test_num):
    k = str(test_num)
    return {"det_ap" + k: res["mAP"], "det_ap50_" + k: res["ap50"], "det_precision50_" + k: res["precision50"],
            "det_recall50_" + k: res["recall50"], "det_detections" + k: res["detections"], "det_boxes" + k: res["boxes"]}
