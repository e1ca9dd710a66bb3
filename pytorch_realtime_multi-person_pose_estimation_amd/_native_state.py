"""Book-keeping shared by the four nn.Module front-ends: native plans, packed-weight arenas and the keys that say what an
arena was packed from (``NativeStateMixin``: network.RtposeVGG, openpose.OpenPose_Model, hourglass.HourglassNet and
shufflenet.Network), and everything the three fronts of the rtpose_net executor do alike with a plan (``NetPlan``,
``NetPlanMixin``: all of the above but shufflenet.Network, which drives another C API).

* Everything is keyed by (device index, compute dtype): a forward on a second GPU - e.g. a replica
  made by ``nn.DataParallel`` (demo/picture_demo.py:47), which shares these dicts by reference
  because ``replicate`` shallow-copies ``__dict__`` - gets its own arena and plans and never evicts
  or re-packs another device's.  One lock serialises plan creation and weight packing.
* An arena is re-packed when a parameter / buffer changed.  ``Tensor._version`` and ``data_ptr()``
  catch ``load_state_dict``, optimiser steps, ``.to()`` / ``.cuda()``; they do NOT see writes made
  through ``.data`` (``p.data.copy_()``, ``p.data.fill_()`` never bump ``_version``).  So
  ``load_state_dict`` and ``_apply`` also bump an explicit epoch, ``invalidate_weights()`` is public
  for code that mutates ``.data``, and ``always_resync = True`` re-packs on every forward.
"""
import collections
import ctypes as C
import threading

import torch

from . import _capi
from ._capi import lib, check, ptr, current_stream

# Plans (one per input shape) keep their activation workspace alive: ~0.22 GB per 368 x 368 image for
# rtpose_vgg in fp32.  An MI355X has 288 GB, and an evaluation run over mixed-size images wants one
# plan per (batch, padded size) bucket, so the cache is bounded by BYTES per device, not by count.
MAX_WORKSPACE_BYTES_PER_DEVICE = 128 << 30
MAX_PLANS_PER_DEVICE = 256
# ... and by what the device really has: at most this fraction of its total memory goes to cached plans (a smaller or
# shared GPU gets a proportionally smaller cache), and an allocation failure evicts the oldest plans and retries.
MAX_WORKSPACE_FRACTION = 0.45

# attributes that hold device memory, native handles or locks: never copied / pickled (each copy builds its own)
_NATIVE_ATTRS = ('_plans', '_weights', '_weights_key', '_weights_epoch', '_native_lock', '_last_input')


class NativeStateMixin(object):
    def _init_native_state(self):
        self._plans = {}         # (n, h, w, device index, dtype) -> plan
        self._weights = {}       # arena key, (device index, dtype) unless NetPlanMixin._arena says otherwise -> packed
                                 # weight arena (torch tensor)
        self._weights_key = {}   # arena key -> what the arena was packed from
        self._weights_epoch = [0]   # boxed: shared with DataParallel replicas like the dicts above
        self._native_lock = threading.RLock()
        self.always_resync = False

    # ---- copy / pickle: copy.deepcopy(model), torch.save(model) and multiprocessing spawn see the parameters and the
    # settings, never the native state (an RLock cannot be pickled, plans and arenas belong to one process and device)
    def __getstate__(self):
        state = self.__dict__.copy()
        for k in _NATIVE_ATTRS:
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        resync = state.get('always_resync', False)
        super(NativeStateMixin, self).__setstate__(state)
        self._init_native_state()
        self.always_resync = resync

    def invalidate_weights(self):
        """Force a re-pack of the native weight arenas on the next forward.  Needed after in-place
        edits through ``.data`` (they leave ``Tensor._version`` untouched); harmless otherwise."""
        with self._native_lock:
            self._weights_epoch[0] += 1
        return self

    def load_state_dict(self, *args, **kwargs):
        r = super(NativeStateMixin, self).load_state_dict(*args, **kwargs)
        self.invalidate_weights()
        return r

    def _apply(self, fn, *args, **kwargs):
        r = super(NativeStateMixin, self)._apply(fn, *args, **kwargs)
        if hasattr(self, "_native_lock"):
            self.invalidate_weights()
        return r

    def _params_key(self, tensors):
        return (self._weights_epoch[0],) + tuple((t._version, t.data_ptr()) for t in tensors)

    def _workspace_cap(self, dev):
        try:
            _, total = torch.cuda.mem_get_info(dev)
            return min(MAX_WORKSPACE_BYTES_PER_DEVICE, int(total * MAX_WORKSPACE_FRACTION))
        except Exception:
            return MAX_WORKSPACE_BYTES_PER_DEVICE

    def _build_plan(self, key, factory):
        """Create a plan with ``factory()`` and cache it under ``key``; when the device cannot hold its workspace
        the oldest cached plans of that device are dropped and the allocation is retried."""
        dev = key[3]
        while True:
            try:
                plan = factory()
                break
            except torch.cuda.OutOfMemoryError:
                mine = [k for k in self._plans if k[3] == dev]
                if not mine:
                    raise
                self._plans.pop(mine[0])
                torch.cuda.empty_cache()
        self._remember_plan(key, plan)
        return plan

    def _remember_plan(self, key, plan):
        dev = key[3]
        mine = [k for k in self._plans if k[3] == dev]          # insertion order: oldest first
        size = lambda p: p.workspace.numel() * p.workspace.element_size()   # noqa: E731
        total = sum(size(self._plans[k]) for k in mine) + size(plan)
        cap = self._workspace_cap(dev)
        while mine and (total > cap or len(mine) >= MAX_PLANS_PER_DEVICE):
            total -= size(self._plans.pop(mine.pop(0)))          # evict plans of THIS device only
        self._plans[key] = plan


def _bn_affine64(bn):
    """Inference BatchNorm2d as y = scale * x + shift, float64, with the module's own eps."""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return scale, bn.bias.detach().double() - bn.running_mean.detach().double() * scale


def bn_scale_shift(bn):
    """(scale, shift) of an inference BatchNorm2d as fp32 vectors (float64 arithmetic)."""
    scale, shift = _bn_affine64(bn)
    return scale.float(), shift.float()


def fold_bn(weight, bias, bn):
    """Filters and bias of ``bn(conv(x))`` as one conv: w * scale[cout], b * scale + shift."""
    scale, shift = _bn_affine64(bn)
    w = weight.detach().double() * scale.view(-1, 1, 1, 1)
    b = (bias.detach().double() if bias is not None else torch.zeros_like(scale)) * scale + shift
    return w.float(), b.float()


class NetPlan(object):
    """One native rtpose_net executor instance (fixed N, H, W) + its workspace, bound to the weight arena `weights` that
    its front keeps under `wkey`.  Takes over `handle` (what a front's ``_create`` returned)."""

    def __init__(self, handle, n, h, w, weights, device, dtype, wino, wkey, stride):
        self.handle = handle
        self.shape = (n, h, w)
        self.dtype = dtype
        self.wino = wino
        self.wkey = wkey
        ws_bytes = lib.rtpose_net_workspace_bytes(handle)
        self.workspace = torch.empty(ws_bytes // 4 + 64, dtype=torch.float32, device=device)
        check(lib.rtpose_net_bind(handle, ptr(self.workspace), ws_bytes, ptr(weights),
                                  weights.numel() * 4, 1, current_stream()), "rtpose_net_bind")
        self.h3 = h // stride       # size of the output maps
        self.w3 = w // stride

    def __del__(self):
        try:
            lib.rtpose_net_destroy(self.handle)
        except Exception:
            pass


# One conv of a front, as _sync_weights loads it: `name` the conv's state_dict prefix, `bn` a BatchNorm2d to fold behind
# the conv, `prelu` (state_dict prefix, nn.PReLU) that follows it, `preact` (state_dict prefix, BatchNorm2d) that the
# conv reads its input through; None where there is none.
ConvRecord = collections.namedtuple('ConvRecord', 'name conv bn prelu preact')


class NetPlanMixin(object):
    """What the three fronts of the rtpose_net executor (network.RtposeVGG, openpose.OpenPose_Model,
    hourglass.HourglassNet) do alike: find or create the plan of an input shape and its weight arena, pack the module's
    parameters into the arena when they changed, enqueue a forward, hand out the maps, report the per-conv arithmetic
    and the device error word.  A front supplies what differs:

    * ``_front_name`` (for the refusals), ``_plan_stride`` (input pixels per output pixel), ``_probe_hw`` (the smallest
      input a plan can be created for; a plan of that size tells the arena's size), ``_wino`` / ``_WINO_DEFAULT`` (the
      front's ``set_winograd`` tuple and its initial value);
    * ``_create(n, h, w, dtype, wino)`` -> a checked native handle, ``_out_channels(which)``;
    * ``_convs()`` (entries whose first element is the conv's state_dict prefix, in the executor's index order) and
      ``_conv_record(entry)`` -> ConvRecord;
    * where the defaults below do not fit: ``_plan_options()``, ``_arena(index, dtype, wino)``, ``_check_ready()``."""

    # ---- what a front may override ------------------------------------------
    def _plan_options(self):
        """(dtype, wino) of the plans created from now on"""
        return _capi.DTYPE_F32, self._wino

    def _arena(self, index, dtype, wino):
        """(key of the weight arena that plans with these options on device `index` bind to, `wino` of the probe plan
        that tells its size).  Plans of a module share the weight arena of their (device, dtype)."""
        return (index, dtype), self._WINO_DEFAULT

    def _check_ready(self):
        """Raises where the module is in no state to run natively."""

    # ---- plans, arenas, weights ----------------------------------------------
    @staticmethod
    def _parse_winograd3(winograd3):
        """``set_winograd(winograd3=)`` of every front -> rtpose_net_options.winograd3"""
        if winograd3 is None:
            return _capi.WINO_DEFAULT
        if winograd3 == 'auto':
            return _capi.WINO3_AUTO
        if winograd3 in (1, 2):        # (True == 1)
            return 1
        if winograd3 in (0, 4):        # (False == 0)
            return int(winograd3)
        raise ValueError("winograd3 must be None, False / 0, True / 1 / 2, 4 or 'auto'")

    def _resolve_device(self, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise _capi.RtposeError("%s plans exist only on an MI355X (HIP) device; got %s - there is no CPU fallback"
                                    % (self._front_name, device))
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        return device

    def _arena_bytes(self, dtype, probe_wino):
        """Size of the weight arena that `_arena` gave this probe for (host only)."""
        probe = self._create(1, self._probe_hw, self._probe_hw, dtype, probe_wino)
        try:
            return lib.rtpose_net_weight_bytes(probe)
        finally:
            lib.rtpose_net_destroy(probe)

    def plan_for(self, x):
        if not x.is_cuda:
            raise _capi.RtposeError(
                "%s forward runs only on an MI355X (HIP) device tensor; got a %s tensor - "
                "there is deliberately no CPU fallback" % (self._front_name, x.device))
        n, c, h, w = x.shape
        if c != 3:
            raise _capi.RtposeError("expected NCHW input with 3 channels")
        return self.plan_for_shape(n, h, w, x.device)

    def plan_for_shape(self, n, h, w, device):
        """The executor instance for N x 3 x H x W inputs on `device` (created on first use), its weights up to date;
        also for callers that fill the plan's input buffer themselves (rtpose_preprocess_u8)."""
        self._check_ready()
        device = self._resolve_device(device)
        dtype, wino = self._plan_options()
        key = (n, h, w, device.index, dtype, wino)
        with self._native_lock, torch.cuda.device(device):
            plan = self._plans.get(key)
            if plan is None:
                wkey, probe_wino = self._arena(device.index, dtype, wino)
                weights = self._weights.get(wkey)
                if weights is None:
                    weights = torch.zeros(self._arena_bytes(dtype, probe_wino) // 4 + 64, dtype=torch.float32,
                                          device=device)
                    self._weights[wkey] = weights
                    self._weights_key.pop(wkey, None)
                plan = self._build_plan(key, lambda: NetPlan(self._create(n, h, w, dtype, wino), n, h, w, weights,
                                                             device, dtype, wino, wkey, self._plan_stride))
            self._sync_weights(plan, device)
            self._finalize(plan)
        return plan

    def _sync_weights(self, plan, device):
        """Packs the module's parameters into the plan's arena unless the arena was packed from just these."""
        recs = [self._conv_record(e) for e in self._convs()]
        tensors = []
        for r in recs:
            tensors += [r.conv.weight, r.conv.bias]
            for bn in (r.bn, r.preact[1] if r.preact else None):
                if bn is not None:
                    tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
            if r.prelu:
                tensors.append(r.prelu[1].weight)
        key = self._params_key(tensors)
        if key == self._weights_key.get(plan.wkey) and not self.always_resync:
            return
        n = lib.rtpose_net_num_convs(plan.handle)
        if n != len(recs):
            raise _capi.RtposeError("native plan has %d convs, module has %d" % (n, len(recs)))
        name = C.create_string_buffer(96)
        co, ci, k = C.c_int(), C.c_int(), C.c_int()
        stream = current_stream()
        keep = []  # temporaries stay alive until the stream has consumed them

        def dev(t):
            t = t.detach()
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return ptr(t)

        def same(what, info, i, mine, channels):
            """the plan and the module agree on whether conv i has a PReLU / pre-activation, its name and its width"""
            has = info(plan.handle, i, name, 96)
            if has < 0 or bool(has) != (mine is not None) or (mine is not None and name.value.decode() != mine[0]):
                raise _capi.RtposeError("%s of conv %d mismatch: native %s vs module %s"
                                        % (what, i, name.value, mine and mine[0]))
            if mine is not None and mine[1].weight.numel() != channels:
                raise _capi.RtposeError("%s has %d channels, the conv %d" % (mine[0], mine[1].weight.numel(), channels))
        for i, r in enumerate(recs):
            check(lib.rtpose_net_conv_info(plan.handle, i, name, 96, C.byref(co), C.byref(ci), C.byref(k)))
            if name.value.decode() != r.name or tuple(r.conv.weight.shape) != (co.value, ci.value, k.value, k.value):
                raise _capi.RtposeError("conv %d mismatch: native %s vs module %s" % (i, name.value, r.name))
            same("PReLU", lib.rtpose_net_prelu_info, i, r.prelu, co.value)
            same("pre-activation", lib.rtpose_net_preact_info, i, r.preact, ci.value)
            w, b = (r.conv.weight, r.conv.bias) if r.bn is None else fold_bn(r.conv.weight, r.conv.bias, r.bn)
            check(lib.rtpose_net_load_conv(plan.handle, i, dev(w), dev(b), stream), "rtpose_net_load_conv")
            if r.prelu is not None:
                check(lib.rtpose_net_load_prelu(plan.handle, i, dev(r.prelu[1].weight), stream), "rtpose_net_load_prelu")
            if r.preact is not None:
                sc, sh = bn_scale_shift(r.preact[1])
                check(lib.rtpose_net_load_preact(plan.handle, i, dev(sc), dev(sh), stream), "rtpose_net_load_preact")
        torch.cuda.current_stream().synchronize()
        del keep
        self._weights_key[plan.wkey] = key

    def _finalize(self, plan):
        # fixes the per-layer forms of an 'auto' plan from the filters in the arena (no-op otherwise)
        check(lib.rtpose_net_finalize_weights(plan.handle, current_stream()), "rtpose_net_finalize_weights")

    def read_output(self, plan, which):
        """Output `which` of the last forward (each front says what it numbers how) as a new NCHW fp32 tensor."""
        out = torch.empty((plan.shape[0], self._out_channels(which), plan.h3, plan.w3), dtype=torch.float32,
                          device=plan.workspace.device)
        check(lib.rtpose_net_read_output(plan.handle, which, ptr(out), current_stream()), "rtpose_net_read_output")
        return out

    # ---- what a plan does -----------------------------------------------------
    def conv_numerics(self, plan):
        """[(state_dict prefix, form, (amp F(2x2,3x3), amp F(4,7), amp F(6,7), amp F(4x4,3x3)))] of a plan: form 0 =
        direct kernel, 3 = F(2x2,3x3), 43 = F(4x4,3x3), 4 / 6 / 8 = F(m,7); amp = rtpose_winograd_amplification of the
        loaded filters (0 = n/a)."""
        out = []
        form = C.c_int()
        amp = (C.c_float * 4)()
        for i, entry in enumerate(self._convs()):
            check(lib.rtpose_net_conv_numerics(plan.handle, i, C.byref(form), amp, current_stream()))
            out.append((entry[0], form.value, tuple(amp)))
        return out

    def device_status(self, plan):
        """Device-side error word of a plan (0 = fine; synchronises the stream)."""
        word = C.c_int()
        check(lib.rtpose_net_device_status(plan.handle, C.byref(word), current_stream()))
        return word.value

    def device_status_async(self, plan, pinned_word):
        """Queue the copy of the plan's device error word into `pinned_word` (a pinned int32 tensor of one element)
        on the current stream, without waiting; read it after an event recorded later on that stream."""
        check(lib.rtpose_net_device_status_async(plan.handle, pinned_word.data_ptr(), current_stream()))

    def forward_native(self, x, keep_intermediates=False):
        """Enqueue the forward; returns the plan (outputs stay in its workspace)."""
        if not x.is_cuda:
            self.plan_for(x)  # raises: no CPU fallback
        with torch.cuda.device(x.device):
            plan = self.plan_for(x)
            xin = x.detach()
            if xin.dtype != torch.float32 or not xin.is_contiguous():
                xin = xin.float().contiguous()
            check(lib.rtpose_net_set_keep_intermediates(plan.handle, 1 if keep_intermediates else 0))
            check(lib.rtpose_net_forward(plan.handle, ptr(xin), current_stream()), "rtpose_net_forward")
            self._last_input = xin  # keep alive until the stream has consumed it
        return plan

    def output_view(self, plan, which):
        """(base pointer, Layout, C, H, W) of the final PAF (0) / heat-map (1), in place."""
        base = C.c_void_p()
        lay = _capi.Layout()
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        check(lib.rtpose_net_output_view(plan.handle, which, C.byref(base), C.byref(lay), C.byref(c),
                                         C.byref(h), C.byref(w)))
        return base, lay, c.value, h.value, w.value
