"""One decode through the C ABI into sentinel-filled buffers with a guard region: shared by tests/test_skeleton_gpu.py and
tests/test_decode_crowd_gpu.py."""
import ctypes as C

import torch

SENTINEL = 0x5A5A5A5A
GUARD = 4096        # words behind each buffer that must stay untouched


def run_decode(capi, cuda, heat, paf, cfg, skel=None, flags=0, nms_only=False, lpaf=None):
    """One decode of dense NHWC maps (device tensors) into sentinel-filled buffers of exactly the queried sizes + a guard
    region; skel None = the COCO-18 entry points.  lpaf: the PAF lies in the buffer `paf` under this layout instead of
    densely (the map size is the heat map's).  -> int32 [N, words]."""
    lib = capi.lib
    n, h, w, ch = heat.shape
    if skel is None:
        rb, wb = lib.rtpose_decode_result_bytes(C.byref(cfg), n), lib.rtpose_decode_workspace_bytes(C.byref(cfg), n)
    else:
        rb = lib.rtpose_decode_result_bytes_skel(C.byref(cfg), C.byref(skel), n)
        wb = lib.rtpose_decode_workspace_bytes_skel(C.byref(cfg), C.byref(skel), n)
    assert rb > 0 and wb > 0 and rb % 4 == 0 and wb % 4 == 0, capi.last_error()
    res = torch.full((rb // 4 + GUARD,), SENTINEL, dtype=torch.int32, device=cuda)
    ws = torch.full((wb // 4 + GUARD,), SENTINEL, dtype=torch.int32, device=cuda)
    lheat = capi.Layout.dense(ch, h, w)
    if lpaf is None:
        lpaf = capi.Layout.dense(paf.shape[3], h, w)
    s = capi.current_stream()
    if skel is None and nms_only:
        rc = lib.rtpose_nms_batch_ex(capi.ptr(heat), C.byref(lheat), n, h, w, C.byref(cfg), flags, capi.ptr(res), s)
    elif skel is None:
        rc = lib.rtpose_decode_batch_ex(capi.ptr(heat), C.byref(lheat), capi.ptr(paf), C.byref(lpaf), n, h, w, C.byref(cfg),
                                        flags, capi.ptr(ws), wb, capi.ptr(res), s)
    elif nms_only:
        rc = lib.rtpose_nms_batch_skel(capi.ptr(heat), C.byref(lheat), n, h, w, C.byref(cfg), C.byref(skel), flags,
                                       capi.ptr(res), s)
    else:
        rc = lib.rtpose_decode_batch_skel(capi.ptr(heat), C.byref(lheat), capi.ptr(paf), C.byref(lpaf), n, h, w,
                                          C.byref(cfg), C.byref(skel), flags, capi.ptr(ws), wb, capi.ptr(res), s)
    capi.check(rc, "decode")
    torch.cuda.synchronize()
    assert bool((res[rb // 4:] == SENTINEL).all()), "the result block's guard region was written"
    assert bool((ws[wb // 4:] == SENTINEL).all()), "the workspace's guard region was written"
    return res[:rb // 4].cpu().numpy().reshape(n, -1)
