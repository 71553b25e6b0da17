"""What BackboneEngine and InternEngine share, and what mtp_amd.parallel.DataParallelTrainer relies on: the freshness
state of the GEMM-side weight images, the weight-gradient side stream, and the report of finished bursts of weight gradients to on_block_done."""
import torch

from . import ops


class EngineBase:
    # per engine class (bench.py and the tests assign them on one class at a time): wgrad_side_stream, wgrad_max_jobs, wgrad_keep

    def __init__(self, module, act_dtype):
        self.m = module
        self.act = act_dtype
        self._key = None                # _weights_key the images and packed weights were last made from
        self._images_fresh = None       # _weights_key at which somebody else wrote the images (mark_images_fresh)
        self._wimg = None               # ops.WeightImages; stays None for a model without image entries
        self._wimg_ptrs = None
        self._ln_parts = []
        self._sl_jobs = []

    # ------------------------------------------------------------------ parameters -> GEMM-side images
    def params(self):
        """name -> nn.Parameter (reference state-dict names)."""
        return dict(self.m.named_parameters())

    def _weights_key(self, P):
        return (self.act,) + tuple((p.data_ptr(), p._version) for p in P.values())

    def prepare_weights(self, force=False):
        """Refresh the GEMM-side weight images when a parameter changed: ONE launch over a descriptor table (ops.WeightImages) into persistent buffers that
        _build_weight_images(P) lays out again only when a parameter moved; _fold_sources(P) runs in front of that launch, _pack_weights(P) (the packed
        ConvT / convolution / padded weights nobody else writes) always behind it."""
        P = self.params()
        key = self._weights_key(P)
        if not force and key == self._key:
            return
        ptrs = (self.act,) + tuple(p.data_ptr() for p in P.values())
        if ptrs != self._wimg_ptrs:
            self._build_weight_images(P)
            self._wimg_ptrs = ptrs
        self._fold_sources(P)
        # (the optimizer launch of DataParallelTrainer writes the images itself and says so: mark_images_fresh -- honoured only while no parameter has been
        #  touched through torch since, i.e. the version counters still are what they were then)
        if self._wimg is not None and (force or self._images_fresh != key):
            self._wimg.refresh()
        self._images_fresh = None
        self._pack_weights(P)
        self._key = key

    def _fold_sources(self, P):
        pass

    def invalidate_weights(self):
        """the parameters changed under torch's version counters (optimizer kernel, broadcast, checkpoint load): the next prepare_weights() redoes everything"""
        self._key = None
        self._images_fresh = None

    def mark_images_fresh(self):
        """the GEMM-side weight images have just been written from the current parameters by somebody else (mtp_adamw_weight_images): the next
        prepare_weights() skips its own image launch -- unless a parameter is modified through torch in between"""
        self._images_fresh = self._weights_key(self.params())
        self._key = None

    def fusable_images(self):
        """the images the optimizer launch may write itself (FlatAdamW.fuse_images), or None"""
        return self._wimg

    # ------------------------------------------------------------------ the weight-gradient side stream
    def _wgrad_stream(self):
        if not self.wgrad_side_stream:
            return None
        import mtp_amd
        note = mtp_amd.hw_queue_note()        # once per process: the side stream needs a hardware queue of its own (mtp_amd/__init__.py)
        if note:
            import warnings
            warnings.warn(note, RuntimeWarning, stacklevel=2)
        if int(self.wgrad_side_stream) == 2:      # a stream of the device's lowest priority
            return ops.low_priority_stream(self.dev)
        st = getattr(self, "_wstream", None)
        if st is None or st.device != self.dev:
            st = self._wstream = torch.cuda.Stream(device=self.dev)
        return st

    def warm_streams(self, device):
        """create AND use the weight-gradient side stream now: the HIP runtime hands a stream its hardware queue at first use, in the order of first uses.  A library
        that creates streams of its own in between (RCCL at communicator creation) otherwise pushes the side stream onto the compute stream's queue -- measured in
        round 6: 34.6 -> 47 ms per step when the C-ABI communicator was created before the first backward (tools/probes/native_comm_probe.py)."""
        self.dev = torch.device(device)
        st = self._wgrad_stream()
        if st is not None:
            with torch.cuda.stream(st):
                torch.zeros(1, device=self.dev).add_(1.0)
            st.synchronize()

    def _e(self, *shape, dtype=None):
        return torch.empty(*shape, device=self.dev, dtype=dtype or self.act)

    # ------------------------------------------------------------------ bursts of weight gradients and their report
    def _begin_backward(self, sqn):
        """the queue of this backward pass (self.dev is set): weight gradients are queued and launched in bursts (ops.WgradQueue).  sqn: see BackboneEngine.backward"""
        self._ln_parts = []
        self._sl_jobs = []
        self._wq = wq = ops.WgradQueue(stream=self._wgrad_stream())
        wq.max_jobs = self.wgrad_max_jobs if wq.stream is not None else 0      # (on the current stream a burst should be whole rounds of the CUs)
        wq.sqn = sqn
        self.norm_covered = wq.covered
        self._pending = []     # side-stream mode: (lowest group, launch mark) of the bursts in flight, reported once the current stream has waited for them
        return wq

    def _ln_flush(self):
        if self._ln_parts:
            ops.reduce_rows_deferred(self._ln_parts)
        if self._sl_jobs:
            ops.small_linear_dw_segments_flush(self._sl_jobs)

    def _burst_out(self, group, on_block_done):
        """launch what is queued; `group` (the lowest block / layer of the burst: its group end covers the whole burst) is reported at once on the current
        stream, and in side-stream mode as soon as the current stream has waited for the burst -- all but the wgrad_keep most recent ones"""
        wq, pending = self._wq, self._pending
        wq.flush()
        self._ln_flush()      # (on the current stream: behind the burst on the side stream they cost the whole gain, 35.4 -> 35.7 ms)
        if wq.stream is None:
            if on_block_done is not None:
                on_block_done(group)
            return
        pending.append((group, wq.launched))
        wq.wait(keep=self.wgrad_keep)
        while pending and pending[0][1] <= wq.launched - len(wq.inflight):      # bursts the current stream has waited for
            g = pending.pop(0)[0]
            if on_block_done is not None:
                on_block_done(g)

    def _wait_bursts(self):
        """the current stream waits for every burst still in flight"""
        self._wq.wait()

    def _report_pending(self, on_block_done):
        """after _wait_bursts: the lowest group still unreported covers the rest"""
        if self._pending and on_block_done is not None:
            on_block_done(self._pending[-1][0])
