"""SML loss on MI355X; same signature and return structure as the reference's utils/loss.py compute_loss :5-135
(train_zju.py:459-470 configures 'l1', w_edge = 0, w_unsupervised = 0, single-scale output).  Every loss hyper-parameter of the training scripts
runs on HIP kernels: 'l1' / 'l2' / 'smoothl1', w_lidar_loss, w_smoothness, w_edge (with or without w_smoothness) and w_unsupervised, whose two
medians over `invalid_map_gt` come from an exact on-device radix selection (csrc/rd_select.hip) -- no sort, no host synchronisation, so the
term runs inside a captured step.

w_unsupervised > 0 needs `invalid_map_gt`: the reference's bool tensor (train_zju.py:361 `batch_gt <= 0`), or, as an extension, the float32
ground-truth map itself, selected where <= 0 (sml_main.forward_loss passes the resized ground truth before outlier removal, so no torch
operation is launched for the mask).  As in the reference an empty mask makes the term and the total NaN (the term then adds no gradient), and a
NaN among the selected values makes the medians NaN.  The selection counts in 32-bit integers: fewer than 2^31 pixels per call."""
import torch

from . import engine


def compute_loss(image, output_depth, gt_interp, gt_sparse, loss_func, w_smoothness, sobel_filter_size, validity_map_loss_smoothness,
                 w_lidar_loss, w_edge, invalid_map_gt, w_unsupervised):
    kinds = {'l1': 0, 'l2': 1, 'smoothl1': 2}
    if loss_func not in kinds:
        raise ValueError('No such loss: {}'.format(loss_func))      # utils/loss.py:103
    if isinstance(output_depth, (list, tuple)):
        if len(output_depth) != 1:
            raise NotImplementedError("multi-scale outputs are not produced by MidasNet_small_videpth")
        output_depth = output_depth[0]
    if image.shape[1] != 1:
        raise NotImplementedError("the SML loop passes the 1-channel depth as `image` (train_zju.py:374-376)")
    c = lambda a: a if a.is_contiguous() else a.contiguous()  # noqa: E731
    img, gi, gs = c(image.float()), c(gt_interp.float()), c(gt_sparse.float())
    wts = None if validity_map_loss_smoothness is None else c(validity_map_loss_smoothness.float())
    mask = None
    if w_unsupervised > 0.0:
        if invalid_map_gt is None:
            raise ValueError("w_unsupervised > 0 needs invalid_map_gt (train_zju.py:361: batch_gt <= 0)")
        if invalid_map_gt.shape != output_depth.shape:
            raise ValueError("invalid_map_gt must have the shape of the output depth")
        if invalid_map_gt.dtype == torch.bool:
            mask = c(invalid_map_gt).view(torch.uint8)      # the same memory: no kernel
        elif invalid_map_gt.dtype == torch.float32:
            mask = c(invalid_map_gt)                        # a ground-truth map: selected where <= 0
        else:
            raise ValueError("invalid_map_gt must be a bool tensor (or a float32 ground-truth map, selected where <= 0)")

    def run(pred):
        p = pred if pred.is_contiguous() else engine.alias(pred, pred.contiguous())
        loss, info, uinfo = engine.sml_loss(p, img, gi, gs, wts, float(w_lidar_loss), float(w_smoothness), float(w_edge), int(sobel_filter_size),
                                            kinds[loss_func], mask, float(w_unsupervised) if mask is not None else 0.0)
        run.info, run.uinfo = info, uinfo
        return loss
    loss = engine.run_region(run, (output_depth,), [])
    info, uinfo = run.info, run.uinfo
    loss_info = {'loss': loss, 'loss_supervised': info[1], 'loss_lidar': info[2] if w_lidar_loss > 0 else 0.0,
                 'loss_smoothness': info[3], 'loss_edge': info[4], 'loss_unsupervised': uinfo[0] if uinfo is not None else 0.0}
    return loss, loss_info
