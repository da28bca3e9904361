"""CPU restatement of the seg programs' mask assembly (process_mask's coefficient loop and its get_downscale_rect:
yolov5/src/postprocess.cpp:94-120, yolov8/yolov8_seg.cpp:17-53), the reference of trtx_seg_masks.  The rect is computed in fp32
exactly as written there; the values in fp64 (or in fp32, sequentially, with dtype=np.float32).  As in the kernel, the rect is
intersected with the plane, a rect with a non-finite edge is empty and edges saturate at +-2^29.  Not a test module."""
import numpy as np

F = np.float32
SAT = 2 ** 29


def c_round(v):
    """C round() on an fp32 value: half away from zero"""
    t = np.trunc(v)
    return F(t + np.sign(v) * F(abs(F(v - t)) >= F(0.5)))


def downscale_rect(bbox, box_format, scale, net_w, net_h):
    """(x, y, width, height) as ints, or None for a non-finite edge.  All arithmetic in fp32."""
    b = [F(v) for v in bbox[:4]]
    s = F(scale)
    with np.errstate(all="ignore"):
        if box_format == 0:
            left, top = F(b[0] - F(b[2] / F(2))), F(b[1] - F(b[3] / F(2)))
            right, bottom = F(b[0] + F(b[2] / F(2))), F(b[1] + F(b[3] / F(2)))
        else:
            left, top, right, bottom = b[0], b[1], F(b[0] + b[2]), F(b[1] + b[3])
            left = F(0) if left < 0 else left
            top = F(0) if top < 0 else top
            right = F(net_w) if right > F(net_w) else right
            bottom = F(net_h) if bottom > F(net_h) else bottom
        left, top, right, bottom = F(left / s), F(top / s), F(right / s), F(bottom / s)
        if not all(np.isfinite(v) for v in (left, top, right, bottom)):
            return None
        to_int = c_round if box_format == 0 else np.trunc
        return tuple(int(np.clip(to_int(v), -SAT, SAT)) for v in (left, top, F(right - left), F(bottom - top)))


def clipped_rect(bbox, box_format, scale, net_w, net_h, mask_w, mask_h):
    """[x0, x1) x [y0, y1) inside the plane; (0, 0, 0, 0) when empty"""
    r = downscale_rect(bbox, box_format, scale, net_w, net_h)
    if r is None:
        return 0, 0, 0, 0
    x, y, w, h = r
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + w, mask_w), min(y + h, mask_h)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else (0, 0, 0, 0)


def seg_masks(decode_out, det_floats, box_format, keep_idx, keep_cnt, max_keep, proto, net_h, net_w, dtype=np.float64):
    """decode_out [B, 1 + max_out * det_floats], keep_idx [B, max_out], keep_cnt [B], proto [B, 32, mh, mw].  Returns
    (masks [B, max_keep, mh, mw] in `dtype` with NaN in the slots the kernel does not write, inside [B, max_keep, mh, mw] bool: the
    clipped rects, mag: sum_j |coef_j * proto_j| in fp64 inside the rects, 0 elsewhere)."""
    B, _, mh, mw = proto.shape
    max_out = keep_idx.shape[1]
    scale = net_w // mw
    masks = np.full((B, max_keep, mh, mw), np.nan, dtype)
    inside = np.zeros((B, max_keep, mh, mw), bool)
    mag = np.zeros((B, max_keep, mh, mw), np.float64)
    rec = decode_out[:, 1:].reshape(B, max_out, det_floats)
    for b in range(B):
        for d in range(min(int(keep_cnt[b]), max_keep)):
            r = rec[b, keep_idx[b, d]]
            x0, y0, x1, y1 = clipped_rect(r[:4], box_format, scale, net_w, net_h, mw, mh)
            masks[b, d] = 0
            if x0 == x1:
                continue
            coef = r[6:38].astype(dtype)
            p = proto[b, :, y0:y1, x0:x1].astype(dtype)
            e = np.zeros(p.shape[1:], dtype)
            with np.errstate(all="ignore"):
                for j in range(32):   # ascending, one rounding per product and per sum in fp32
                    e = (e + (coef[j] * p[j]).astype(dtype)).astype(dtype)
                masks[b, d, y0:y1, x0:x1] = (dtype(1) / (dtype(1) + np.exp(-e))).astype(dtype)
                mag[b, d, y0:y1, x0:x1] = np.abs(coef.astype(np.float64)[:, None, None] * p.astype(np.float64)).sum(0)
            inside[b, d, y0:y1, x0:x1] = True
    return masks, inside, mag


def bound(mag):
    """|fp32 kernel - fp64 reference|: the sequential fp32 sum of 32 products (33 roundings of 2^-24 relative to sum |terms|) through a
    function of slope at most 1/4, plus expf and the division"""
    return 33 * 2.0 ** -24 * mag / 4 + 2.0 ** -22


__all__ = ["bound", "c_round", "clipped_rect", "downscale_rect", "seg_masks"]
