"""REGTR network, inference forward, on the MI355X HIP kernels.

Drop-in for the reference's `RegTR` (/root/reference/src/models/regtr.py:22-235): same constructor (`RegTR(cfg)`),
same `forward(batch) -> dict` contract (input lists batch['src_xyz'] / batch['tgt_xyz'], side effect
batch['kpconv_meta'], output keys of regtr.py:218-235), same `state_dict` names and shapes, so a reference checkpoint
loads with `load_state_dict(state['state_dict'])` (demo.py:165).  `compute_loss(pred, batch)` gives the reference's validation /
test losses (regtr.py:237-294) without gradients: the feature terms on regtr_infonce (`feature_loss_type: infonce`) or
regtr_circle_rows (`feature_loss_type: circle`, CircleLossFull with no parameters), the overlap and correspondence terms on
regtr_loss_terms.  `training_step(batch)` trains everything above a frozen KPConv backbone (feat_proj, the cross-encoder, the
correspondence head, the InfoNCE W) with HIP backward kernels: forward_grad / compute_loss_grad / trainable_parameters;
`training_step(batch, train_backbone=True)` also trains the 11 KPConv blocks (KPFEncoder.forward_grad, regtr_amd/encoder_grad.py) --
every parameter the reference trains.  `configure_optimizers` sets the reference's optimiser and scheduler (regtr_amd/optim.py: the fused
clip + AdamW step; harness.train_loop / train.py run the loop).  `validation_step` / `validation_epoch_end` / `test_step`
are the reference's (generic_reg_model.py:82-104, 130-158) with the registration metrics computed on the device (regtr_amd/metrics.py).
`pos_emb_type: learned` puts the reference's PositionEmbeddingLearned in place of the sine table (one launch, regtr_posemb_mlp); its ten
tensors are trained with everything else above the backbone.

The forward enqueues every stage on the current HIP stream with ONE host synchronisation (the data-dependent level
sizes after preprocessing): preprocess -> KPConv encoder -> feat_proj -> 6 cross-encoder layers on packed tokens ->
correspondence head -> fused weighted-Procrustes.
"""
import logging
import threading

import torch
import torch.nn as nn

from . import _lib, context, ops, overlap
from .config import as_config
from .kpconv import KPFEncoder, PreprocessorGPU, _prepared
from .transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer

_TIMEIT = False   # reference: regtr.py:19 -- stage timer (preprocess / encoder / attention+head / pose / total)


class PositionEmbeddingCoordsSine(nn.Module):
    """position_embedding.py:7-50 (parameter free)."""

    def __init__(self, n_dim=1, d_model=256, temperature=10000, scale=None):
        super().__init__()
        if n_dim != 3:
            raise NotImplementedError
        self.n_dim, self.d_model, self.temperature = n_dim, d_model, temperature
        self.scale = 1.0 if scale is None else scale

    def forward(self, xyz):
        return ops.posemb_sine(xyz, self.d_model, self.scale, self.temperature)


class PositionEmbeddingLearned(nn.Module):
    """position_embedding.py:53-72: a five-Linear ReLU MLP 3 -> 32 -> 64 -> 128 -> 256 -> d_model over the coordinates, `mlp` with the
    reference's layer indices (state_dict: mlp.{0,2,4,6,8}.{weight,bias}) and nn.Linear's default initialisation.  forward runs it in
    one launch (ops.posemb_mlp: regtr_posemb_mlp, exact float32); forward_grad is the same bits with a HIP backward."""

    def __init__(self, n_dim=1, d_model=256):
        super().__init__()
        if n_dim != 3:
            raise NotImplementedError(f'PositionEmbeddingLearned: n_dim {n_dim} (only the 3 coordinates of a point are implemented)')
        if d_model % 64 or not 64 <= d_model <= 512:
            raise NotImplementedError(f'PositionEmbeddingLearned: d_model must be a multiple of 64 in [64, 512] (regtr_posemb_mlp), got {d_model}')
        self.n_dim, self.d_model = n_dim, d_model
        self.mlp = nn.Sequential(nn.Linear(n_dim, 32), nn.ReLU(), nn.Linear(32, 64), nn.ReLU(), nn.Linear(64, 128), nn.ReLU(),
                                 nn.Linear(128, 256), nn.ReLU(), nn.Linear(256, d_model))
        self._cache = {}

    def linears(self):
        return [self.mlp[i] for i in (0, 2, 4, 6, 8)]

    def _weights(self):
        """The five (weight in (K, N) layout, bias) pairs ops.posemb_mlp reads: the transposes once per weight version."""
        return [(_prepared(self._cache, ('kn', i), lin.weight, lambda w: w.t().contiguous()), lin.bias.detach())
                for i, lin in enumerate(self.linears())]

    def forward(self, xyz):
        return ops.posemb_mlp(xyz, self._weights())

    def forward_grad(self, xyz):
        """forward(xyz), bit for bit, differentiable in the ten parameters with a HIP backward (head_grad.posemb_forward_grad).
        Refused: CPU tensors, double backward, xyz.requires_grad (coordinates take no gradient)."""
        from . import head_grad
        return head_grad.posemb_forward_grad(self, xyz)


# A-B switch and size gate of the two-stream forward (RegTR._forward)
overlap_preprocessing = True
OVERLAP_MIN_POINTS = 131072


class CorrespondenceRegressor(nn.Module):
    """regtr.py:399-443: coor_mlp (D->D->D->3, ReLU) and conf_logits_decoder (D->1)."""

    def __init__(self, d_embed):
        super().__init__()
        self.coor_mlp = nn.Sequential(nn.Linear(d_embed, d_embed), nn.ReLU(), nn.Linear(d_embed, d_embed), nn.ReLU(),
                                      nn.Linear(d_embed, 3))
        self.conf_logits_decoder = nn.Linear(d_embed, 1)
        self._cache = {}

    def _mlp(self, f):
        """f (M, D) -> (h1, h2, corr (M, 3), logit (M, 1)): the four Linears, the ReLUs in the first two's epilogues."""
        wt = lambda k, lin: _prepared(self._cache, k, lin.weight, lambda w: ops.SplitWeight(w, 'nk'))
        h1 = ops.gemm(f, wt('0', self.coor_mlp[0]), bias=self.coor_mlp[0].bias.detach(), relu=True)
        h2 = ops.gemm(h1, wt('2', self.coor_mlp[2]), bias=self.coor_mlp[2].bias.detach(), relu=True)
        corr = ops.gemm(h2, wt('4', self.coor_mlp[4]), bias=self.coor_mlp[4].bias.detach())
        logit = ops.gemm(f, wt('c', self.conf_logits_decoder), bias=self.conf_logits_decoder.bias.detach())
        return h1, h2, corr, logit

    def forward(self, feats):
        """feats (L, N, D) -> corr (L, N, 3), logit (L, N)."""
        Lyr, N, D = feats.shape
        _, _, corr, logit = self._mlp(feats.view(Lyr * N, D))
        return corr.view(Lyr, N, 3), logit.view(Lyr, N)

    def forward_grad(self, feats):
        """forward(feats), bit for bit, differentiable in feats and in all eight parameters, with a HIP backward
        (regtr_amd/head_grad.py).  Refused: CPU tensors, double backward, d_embed not a multiple of 64."""
        from . import head_grad
        return head_grad.regressor_forward_grad(self, feats)


class CorrespondenceDecoder(nn.Module):
    """regtr.py:299-396 (`direct_regress_coor: False`): correspondences as attention-weighted partner coordinates --
    softmax(q_proj(f [+ pe]) . k_proj(f_partner [+ pe]) / sqrt(D)) @ xyz_partner per decoder layer -- and the overlap logit.
    `q_norm` is a parameter of the reference module that its forward never uses; it is kept for strict loading."""

    def __init__(self, d_embed, use_pos_emb, num_neighbors=0):
        super().__init__()
        if num_neighbors != 0:
            raise NotImplementedError('num_neighbors > 0 (top-k masked attention) is not used by the reference model')
        self.use_pos_emb = use_pos_emb
        self.q_norm = nn.LayerNorm(d_embed)
        self.q_proj = nn.Linear(d_embed, d_embed)
        self.k_proj = nn.Linear(d_embed, d_embed)
        self.conf_logits_decoder = nn.Linear(d_embed, 1)
        self._cache = {}

    def forward_grad(self, *args, **kwargs):
        raise NotImplementedError('CorrespondenceDecoder.forward_grad: the attention-valued head (direct_regress_coor: false) has no '
                                  'backward (regtr_attn_xyz); only CorrespondenceRegressor is differentiable')

    def forward(self, feats, pe, xyz, seg_off, kv_cross, max_len):
        """feats (L, N, D) conditioned features of all clouds, pe (N, D), xyz (N, 3) -> corr (L, N, 3), logit (L, N)."""
        Lyr, N, D = feats.shape
        wt = lambda k, lin: _prepared(self._cache, k, lin.weight, lambda w: ops.SplitWeight(w, 'nk'))
        f2 = torch.stack([ops.add(feats[l], pe) for l in range(Lyr)]) if self.use_pos_emb else feats       # :372-373
        q = ops.gemm(f2.view(Lyr * N, D), wt('q', self.q_proj), bias=self.q_proj.bias.detach())
        k = ops.gemm(f2.view(Lyr * N, D), wt('k', self.k_proj), bias=self.k_proj.bias.detach())
        corr = ops.attn_xyz(q.view(Lyr, N, D), k.view(Lyr, N, D), xyz, seg_off, kv_cross, max_len)         # :374-377
        logit = ops.gemm(feats.reshape(Lyr * N, D), wt('c', self.conf_logits_decoder), bias=self.conf_logits_decoder.bias.detach())
        return corr, logit.view(Lyr, N)


def _throttled(n):
    """Log occurrence no. n?  The first three, then every power of two: a permanent condition stays visible without flooding the log."""
    return n <= 3 or (n & (n - 1)) == 0


class _LossParams(nn.Module):
    """Holds InfoNCELossFull.W (feature_loss.py:261): loaded strictly from reference checkpoints, read by RegTR.compute_loss."""

    def __init__(self, d_embed):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(d_embed, d_embed), requires_grad=False)


def loss_weight_dict(cfg):
    """regtr.py:90-95: {'overlap_i', 'feature_i', 'corr_i', 'feature_un'} -> weight."""
    wd = {}
    for k in ['overlap', 'feature', 'corr']:
        for i in cfg.get(f'{k}_loss_on', [cfg.num_encoder_layers - 1]):
            wd[f'{k}_{i}'] = cfg.get(f'wt_{k}')
    wd['feature_un'] = cfg.wt_feature_un
    if pose_loss_on(cfg):
        wd[f'pose_{cfg.num_encoder_layers - 1}'] = cfg.wt_pose
    return wd


def pose_loss_on(cfg):
    """cfg.wt_pose > 0: the opt-in pose term (losses.PoseCriterion on the last decoder layer's pose; NOT a loss of the reference, whose
    configs have no such key).  Absent or 0: no key, no launch, nothing changes anywhere."""
    return float(cfg.get('wt_pose', 0) or 0) > 0


def _packed_rows(views):
    """Row views (n_k, ...) of one tensor, one per cloud, as ONE (sum n_k, ...) tensor: a view when they lie back to back in memory
    (what RegTR.forward returns), else a copy."""
    v0 = views[0]
    n = sum(int(v.shape[0]) for v in views)
    row = v0.stride(0) if v0.dim() else 1
    at = v0.data_ptr()
    base = v0.untyped_storage().data_ptr()
    adjacent = all(v.stride() == v0.stride() and v.dtype == v0.dtype and v.untyped_storage().data_ptr() == base for v in views)
    for v in views:
        if not adjacent:
            break
        if v.shape[0] and v.data_ptr() != at:
            adjacent = False
        at += int(v.shape[0]) * row * v.element_size()
    if adjacent:
        return v0.as_strided((n,) + tuple(v0.shape[1:]), v0.stride(), v0.storage_offset())
    return torch.cat([v.contiguous() for v in views], dim=0)


class RegTR(nn.Module):
    def __init__(self, cfg, *args, **kwargs):
        super().__init__()
        cfg = as_config(cfg)
        self.cfg = cfg
        self.logger = logging.getLogger(self.__class__.__name__)
        self.preprocessor = PreprocessorGPU(cfg)                                  # regtr.py:29
        self.kpf_encoder = KPFEncoder(cfg, cfg.d_embed)                           # :34
        self.feat_proj = nn.Linear(self.kpf_encoder.encoder_skip_dims[-1], cfg.d_embed, bias=True)   # :36
        pos_emb_type = cfg.get('pos_emb_type', 'sine')                            # :41-47
        if pos_emb_type == 'sine':
            self.pos_embed = PositionEmbeddingCoordsSine(3, cfg.d_embed, scale=cfg.get('pos_emb_scaling', 1.0))
        elif pos_emb_type == 'learned':
            self.pos_embed = PositionEmbeddingLearned(3, cfg.d_embed)
        else:
            raise NotImplementedError(f"pos_emb_type {pos_emb_type!r}: choose 'sine' or 'learned'")
        encoder_layer = TransformerCrossEncoderLayer(                             # :52-59
            cfg.d_embed, cfg.nhead, cfg.d_feedforward, cfg.dropout, activation=cfg.transformer_act,
            normalize_before=cfg.pre_norm, sa_val_has_pos_emb=cfg.sa_val_has_pos_emb,
            ca_val_has_pos_emb=cfg.ca_val_has_pos_emb, attention_type=cfg.attention_type)
        encoder_norm = nn.LayerNorm(cfg.d_embed) if cfg.pre_norm else None
        # cfg.compute_dtype (not a reference key).  Every dense contraction runs on the 16-bit matrix cores with EXACT operand splits and
        # float32 accumulation.  'fp32' (default): the f16 PAIR split -- x = h0 + h1 / 2048, three f16 MFMA terms, error ~2^-22 per
        # product, 22-bit operands that must stay below f16's 65504 -- in the split GEMMs and the attention core, the six-term bf16 split
        # (~2^-24) in the one-shot strip / block-tail kernels of the shallow levels and wherever the f16 format does not serve a launch.
        # RANGE: InstanceNorm / LayerNorm outputs and their gathered sums sit far below the limit with sane weights (largest |A| 116 on
        # the benchmark workload), but nothing bounds a checkpoint's FFN activations, so it is CHECKED: weights once per version
        # (ops.SplitWeight.f16_ok), activations by the kernels themselves -- a non-finite f16 pair product or pose sets a bit in a
        # device status word that forward() reads once, at its end, and on a trip the forward is re-run in 'fp32x3' arithmetic and the
        # event logged (cfg.f16_range_check: False skips the check and its end-of-forward wait).  Validated against the real reference
        # module's outputs on the goldens in parity mode (worst 2.6e-5, bar 1e-4) and on the benchmarked batch (bench.py's `parity`).
        # 'fp32x3' = six bf16 terms everywhere (float32's operand range, no f16); 'bf16x2' = three bf16 terms in the cross-encoder's
        # Linears without the f16 pair (round-2 callers); 'bf16' = plain bf16 operands with float32 accumulation / softmax in the
        # cross-encoder's Linears and attention core (BASELINE configs[1]; encoder, head, pose as 'fp32').
        dt = cfg.get('compute_dtype', 'fp32')
        if dt not in ('fp32', 'fp32x3', 'bf16', 'bf16x2'):
            raise NotImplementedError(f'compute_dtype {dt!r}: choose fp32, fp32x3, bf16x2 or bf16')
        # (bf16 planes per operand where the f16 pair does not serve a launch: 'fp32' then means six terms, like 'fp32x3')
        encoder_layer.gemm_planes = {'fp32': 3, 'fp32x3': 3, 'bf16x2': 2, 'bf16': 1}[dt]
        encoder_layer.attn_precision = 1 if dt == 'bf16' else (3 if dt == 'fp32' else 0)      # ops.mha's codes
        self._f16_pair = dt in ('fp32', 'bf16')      # ('bf16': the encoder / head GEMMs, which stay float32-grade)
        self._range_check = bool(cfg.get('f16_range_check', True))
        self.f16_range_fallbacks = 0          # forwards re-run in fp32x3 arithmetic because an f16 pair operand left the format's range
        self.nonfinite_pose_forwards = 0      # forwards whose pose came out non-finite with every f16 pair product finite (bad inputs / weights)
        self.transformer_encoder = TransformerCrossEncoder(encoder_layer, cfg.num_encoder_layers, encoder_norm,
                                                           return_intermediate=True)
        if cfg.get('direct_regress_coor', False):                                 # :68-73
            self.correspondence_decoder = CorrespondenceRegressor(cfg.d_embed)
        else:
            self.correspondence_decoder = CorrespondenceDecoder(cfg.d_embed, cfg.corr_decoder_has_pos_emb)
        loss_type = cfg.get('feature_loss_type', 'infonce')
        if loss_type == 'infonce':                                                # :79-81
            self.feature_criterion = _LossParams(cfg.d_embed)
            self.feature_criterion_un = _LossParams(cfg.d_embed)
        elif loss_type == 'circle':                                               # :82-84: ONE criterion, no parameters
            from .losses import CircleLossFull
            self.feature_criterion = self.feature_criterion_un = CircleLossFull('euclidean', r_p=cfg.get('r_p', 0.125),
                                                                                r_n=cfg.get('r_n', 0.25))
        else:
            raise NotImplementedError(f"feature_loss_type {loss_type!r}: choose 'infonce' or 'circle'")        # :85-86
        self.weight_dict = loss_weight_dict(cfg) if 'wt_feature_un' in cfg else None        # :90-95 (configs with a losses section)
        self._cache = {}
        self.last_timings = None
        self._params_checked = False

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() / .half() / .double(): re-validate at the next forward
        self._params_checked = False
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._params_checked = False
        return super().load_state_dict(*args, **kwargs)

    def _status_word(self, dev):
        """(device int32[1], pinned host int32[1]) the kernels of ONE forward OR bits into.  One pair per (host thread, HIP stream): two
        threads -- or two streams -- driving the SAME model each zero, fill and read their own word, so one forward can neither erase nor
        steal another's overflow bit (a forward is complete on its stream before the next one on that stream zeroes the word)."""
        key = ('status', dev, threading.get_ident(), _lib.stream())
        ent = self._cache.get(key)
        if ent is None:
            if sum(1 for k in self._cache if isinstance(k, tuple) and k and k[0] == 'status') > 64:       # dead threads / streams
                for k in [k for k in self._cache if isinstance(k, tuple) and k and k[0] == 'status']:
                    del self._cache[k]
            ent = self._cache[key] = (torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32).pin_memory())
        return ent

    def _ones(self, n, dev):
        """RegTR's input features (regtr.py:136: ones, one per point) as a view of a cached buffer: constant data, a fill kernel and an
        allocation less per forward.  One buffer per (device, stream), like the status word: created and regrown in stream order, so a second
        thread / stream driving this model can neither read it before its fill kernel ran nor lose it to another stream's regrow."""
        key = ('ones', dev, torch.cuda.current_stream(dev).cuda_stream)
        ent = self._cache.get(key)
        if ent is None or ent.shape[0] < n:
            ent = self._cache[key] = torch.ones((max(n, 1) * 5 // 4 + 16, 1), dtype=torch.float32, device=dev)
        return ent[:n]

    def _side_stream(self, dev):
        """The pyramid's stream (large batches: levels 1-3 are built under the level-0 blocks).  HIGH priority, not for the priority: HIP maps
        the streams of one priority onto a small pool of hardware queues, and a stream that lands on the main stream's queue is serialised
        behind it.  That happened as soon as the process also held an RCCL communicator (its streams shift the mapping): a 192-pair forward
        79.98 ms under a world-1 process group against 77.84 ms without, the rocprofv3 trace showing no overlap at all (busy 78.2 ms inside 79.5 ms
        of wall time, against 84.4 inside 76.6).  A high-priority stream draws from its own queue pool: 78.20 / 77.94 ms (profiles/r05_z_dist_stream.txt)."""
        return _prepared(self._cache, ('side_stream', dev), self.feat_proj.bias,
                         lambda _: torch.cuda.Stream(device=dev, priority=-1))

    @staticmethod
    def _record_meta(meta, stream):
        """Pyramid tensors are allocated on the side stream and read on `stream`: tell the caching allocator."""
        for key in ('points', 'neighbors', 'pools', '_neighbors_i32', '_pools_i32', '_seg_off'):
            for t in meta[key]:
                t.record_stream(stream)

    @property
    def device(self):
        return next(self.parameters()).device

    # (forward's placement checks and its status-word / fp32x3 fallback policy have a twin for encode_clouds / register below:
    #  _check_placement and _run_checked.  A change to the policy here belongs there too.)
    @torch.no_grad()
    def forward(self, batch):
        dev = batch['src_xyz'][0].device
        if dev.type != 'cuda':
            raise RuntimeError('regtr_amd.RegTR runs on an MI355X (HIP) device only; there is no CPU path')
        clouds = batch['src_xyz'] + batch['tgt_xyz']
        if not self._params_checked:        # once per parameter (re)placement: _apply() below resets it
            bad = [n for n, p in self.named_parameters() if p.dtype != torch.float32]
            if bad:
                raise RuntimeError(f'regtr_amd.RegTR computes in float32; non-float32 parameters: {bad[:3]} ...')
            self._model_device = next(self.parameters()).device
            self._params_checked = True
        if any(p.device != dev for p in clouds) or self._model_device != dev:
            raise RuntimeError(f'RegTR.forward: the model ({self._model_device}) and every input cloud must live on one GPU ({dev})')
        # kernels go to torch's current stream of the CURRENT device: the context makes the tensors' device current for the whole
        # forward and carries the operand format / status word to every launch (thread-local: regtr_amd/context.py)
        check = self._f16_pair and self._range_check
        with context.forward(dev, f16_pair=self._f16_pair, status=None) as ctx:
            if not check:
                return self._forward(batch, dev)
            st_dev, st_host = self._status_word(dev)         # (inside the context: the launch device is current, the stream is this thread's)
            ctx.status = st_dev
            st_dev.zero_()
            out = self._forward(batch, dev)
            st_host.copy_(st_dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            done.synchronize()                  # the one wait at the end of a forward: the status word (4 bytes, pinned)
            bits = int(st_host[0])
        if bits == 0:
            return out
        if not bits & context.STATUS_F16_RANGE:
            # only the pose is non-finite: the f16 pair products were all finite, so the arithmetic is not the cause -- a NaN / Inf in the
            # input clouds or the weights, or a degenerate pair.  A re-run in fp32x3 would return the same NaN at twice the cost.
            self.nonfinite_pose_forwards += 1
            if self.nonfinite_pose_forwards == 1 and self._f16_pair:
                # ... the FIRST time, checked instead of assumed: one re-run with six-term bf16 splits.  A finite pose there means an f16 pair
                # kernel produced a degenerate result WITHOUT raising its range bit -- a defect to report, and the finite result is returned.
                with context.forward(dev, f16_pair=False, force_x3=True, status=None):
                    again = self._forward(batch, dev)
                if bool(torch.isfinite(again['pose']).all()):
                    self.logger.error("non-finite pose with NO f16 range bit set, but the fp32x3 re-run is finite: an f16 pair kernel missed its "
                                      "range report (status %d) -- returning the fp32x3 result; set cfg.compute_dtype: fp32x3 and report this", bits)
                    return again
                self.logger.warning('non-finite pose (status %d): the fp32x3 re-run is non-finite too -- the inputs or the checkpoint hold NaN / Inf', bits)
            if _throttled(self.nonfinite_pose_forwards):
                self.logger.warning('non-finite pose in the output (status %d; forward no. %d with this condition): every f16 pair product was '
                                    'finite, so check the input clouds and the checkpoint for NaN / Inf -- returned as is, not re-run',
                                    bits, self.nonfinite_pose_forwards)
            return out
        # an operand left f16's range: the same forward in fp32x3 arithmetic -- float32's range
        self.f16_range_fallbacks += 1
        if _throttled(self.f16_range_fallbacks):
            self.logger.warning('f16 pair operand range exceeded (status %d; fallback no. %d) -- forward re-run with six-term bf16 splits '
                                "(compute_dtype 'fp32x3' arithmetic, twice the cost of this forward); set cfg.compute_dtype: fp32x3 to skip "
                                'the first attempt', bits, self.f16_range_fallbacks)
        with context.forward(dev, f16_pair=False, force_x3=True, status=None):
            return self._forward(batch, dev)

    def _kv_tables(self, B, dev):
        """(kv_self, kv_cross) (2B,) int32: the cloud each cloud's self- / cross-attention reads (its own; its pair's partner)."""
        kv_self = _prepared(self._cache, ('kv_self', B, dev), self.feat_proj.bias,
                            lambda _: torch.arange(2 * B, dtype=torch.int32, device=dev))
        kv_cross = _prepared(self._cache, ('kv_cross', B, dev), self.feat_proj.bias,
                             lambda _: torch.cat([torch.arange(B, 2 * B), torch.arange(0, B)]).to(torch.int32).to(dev))
        return kv_self, kv_cross

    def _backbone(self, batch, dev, ev=None, train=False):
        """preprocess (regtr.py:117-122) + KPConv encoder (regtr.py:136) -> (feats_un, kpconv_meta); sets batch['kpconv_meta'].
        train: the pyramid without gradient on ONE stream, the encoder through KPFEncoder.forward_grad inside autograd."""
        clouds = batch['src_xyz'] + batch['tgt_xyz']
        n0 = sum(int(p.shape[0]) for p in clouds)
        n_l0 = self.kpf_encoder.level0_blocks()
        two_streams = (overlap_preprocessing and n_l0 > 0 and not ev and not self.cfg.get('kpconv_ref_row_order', False))
        if two_streams and n0 >= OVERLAP_MIN_POINTS and not train:
            # Large batches: the pyramid is built on a second HIP stream, and the level-0 blocks -- which need only level 0's conv
            # table and sizes the host already knows -- start on the main stream as soon as that table exists: the other 2.4 ms of
            # pyramid building (latency-bound small kernels) run under 6 ms of bandwidth-bound level-0 convolution.
            main = torch.cuda.current_stream()
            side = self._side_stream(dev)
            ev0 = torch.cuda.Event()
            side.wait_stream(main)                                   # the inputs
            with torch.cuda.stream(side):
                state = self.preprocessor.enqueue(clouds, level0_event=ev0)
            meta0 = self.preprocessor.level0_meta(state)
            for t in (meta0['points'][0], meta0['_neighbors_i32'][0], meta0['_seg_off'][0]):
                t.record_stream(main)                                # allocated on `side`, read on `main`
            main.wait_event(ev0)
            feats0 = torch.ones_like(meta0['points'][0][:, 0:1])
            x, skips = self.kpf_encoder(feats0, meta0, 0, n_l0)
            kpconv_meta = self.preprocessor.finish(state)            # host + main wait for the pyramid's `done` event only
            if kpconv_meta is None:      # a level filled its capacity (rare): the pyramid once more, here, at full capacity -- the level-0
                kpconv_meta = self.preprocessor(clouds)          # blocks already enqueued read level 0 only, which is never truncated
            else:
                self._record_meta(kpconv_meta, main)
            batch['kpconv_meta'] = kpconv_meta
            feats_un, _ = self.kpf_encoder(x, kpconv_meta, n_l0, None, skips)
        else:
            if train:
                with torch.no_grad():
                    kpconv_meta = self.preprocessor(clouds)
            else:
                kpconv_meta = self.preprocessor(clouds)
            batch['kpconv_meta'] = kpconv_meta
            # (small batches -- a pair or two per forward -- run ONE stream: the level-0 blocks overlapped with pyramid levels 1-3 on a second
            #  stream, with the pyramid sequenced from C in two phases, measured 2.46 vs 2.38 ms per pair: docs/NEGATIVES.md, round 5)
            feats0 = self._ones(kpconv_meta['points'][0].shape[0], dev)
            if ev: ev[1].record()
            if train:
                feats_un = self.kpf_encoder.forward_grad(feats0, kpconv_meta)
            else:
                feats_un, _ = self.kpf_encoder(feats0, kpconv_meta)
        return feats_un, kpconv_meta

    def _forward(self, batch, dev):
        B = len(batch['src_xyz'])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if _TIMEIT else None
        if ev: ev[0].record()
        feats_un, kpconv_meta = self._backbone(batch, dev, ev)
        slens_c = kpconv_meta['_lens_host'][-1]
        src_slens_c, tgt_slens_c = slens_c[:B], slens_c[B:]
        if ev: ev[2].record()

        # ---- projection, positional embedding, cross-encoder on packed tokens (regtr.py:145-166)
        wt = _prepared(self._cache, 'feat_proj', self.feat_proj.weight, lambda w: ops.SplitWeight(w, 'nk'))
        both_feats_un = ops.gemm(feats_un, wt, bias=self.feat_proj.bias.detach())
        xyz_c = kpconv_meta['points'][-1]
        seg_c = kpconv_meta['_seg_off'][-1]
        pe = self.pos_embed(xyz_c) if self.cfg.transformer_encoder_has_pos_emb else None
        kv_self, kv_cross = self._kv_tables(B, dev)
        feats_cond = self.transformer_encoder(both_feats_un, pe, seg_c, kv_self, kv_cross, max(slens_c))   # (L, N, D)

        # ---- correspondence head (regtr.py:168) and pose (regtr.py:185-203)
        if isinstance(self.correspondence_decoder, CorrespondenceRegressor):
            corr, logit = self.correspondence_decoder(feats_cond)
        else:
            pe_c = pe if pe is not None else self.pos_embed(xyz_c)
            corr, logit = self.correspondence_decoder(feats_cond, pe_c, xyz_c, seg_c, kv_cross, max(slens_c))
        if ev: ev[3].record()
        pose = ops.weighted_procrustes(xyz_c, corr, logit, seg_c, B)
        if ev:
            ev[4].record()
            torch.cuda.synchronize()
            self.last_timings = {'preprocess': ev[0].elapsed_time(ev[1]) / 1e3, 'encoder': ev[1].elapsed_time(ev[2]) / 1e3,
                                 'attention': ev[2].elapsed_time(ev[3]) / 1e3, 'pose': ev[3].elapsed_time(ev[4]) / 1e3,
                                 'total': ev[0].elapsed_time(ev[4]) / 1e3}

        # ---- unpack into the reference's per-pair lists (views, no copies)
        off = [0]
        for n in slens_c:
            off.append(off[-1] + n)
        sl = lambda c: slice(off[c], off[c + 1])
        logit3 = logit.unsqueeze(-1)
        outputs = {
            'src_feat_un': tuple(both_feats_un[sl(b)] for b in range(B)),
            'tgt_feat_un': tuple(both_feats_un[sl(B + b)] for b in range(B)),
            'src_feat': [feats_cond[:, sl(b)] for b in range(B)],          # List(B) of (N_pred, N_src, D)
            'tgt_feat': [feats_cond[:, sl(B + b)] for b in range(B)],
            'src_kp': tuple(xyz_c[sl(b)] for b in range(B)),
            'src_kp_warped': [corr[:, sl(b)] for b in range(B)],
            'tgt_kp': tuple(xyz_c[sl(B + b)] for b in range(B)),
            'tgt_kp_warped': [corr[:, sl(B + b)] for b in range(B)],
            'src_overlap': [logit3[:, sl(b)] for b in range(B)],
            'tgt_overlap': [logit3[:, sl(B + b)] for b in range(B)],
            'pose': pose,
        }
        return outputs

    # ------------------------------------------------------------------------------------------ encode each cloud once, register many pairs
    def _check_placement(self, dev, tensors, what):
        """forward's checks, for the calls below: float32 parameters, the model and every tensor on one GPU."""
        if dev.type != 'cuda':
            raise RuntimeError('regtr_amd.RegTR runs on an MI355X (HIP) device only; there is no CPU path')
        if not self._params_checked:
            bad = [n for n, p in self.named_parameters() if p.dtype != torch.float32]
            if bad:
                raise RuntimeError(f'regtr_amd.RegTR computes in float32; non-float32 parameters: {bad[:3]} ...')
            self._model_device = next(self.parameters()).device
            self._params_checked = True
        if any(t.device != dev for t in tensors) or self._model_device != dev:
            raise RuntimeError(f'RegTR.{what}: the model ({self._model_device}) and every input must live on one GPU ({dev})')

    def _run_checked(self, dev, run, what, pose_of=None):
        """run() under forward's arithmetic policy: the model's compute_dtype, the f16 status word read ONCE at the end (the call's only
        host wait of its own), on a range trip the whole of run() again in fp32x3 arithmetic (f16_range_fallbacks), a non-finite pose
        with every f16 product finite reported and returned as it is (nonfinite_pose_forwards; the first time, as in forward, checked
        by one fp32x3 re-run whose finite result would be returned).  pose_of: run()'s result -> its pose tensor."""
        check = self._f16_pair and self._range_check
        with context.forward(dev, f16_pair=self._f16_pair, status=None) as ctx:
            if not check:
                return run()
            st_dev, st_host = self._status_word(dev)
            ctx.status = st_dev
            st_dev.zero_()
            out = run()
            st_host.copy_(st_dev, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
            bits = int(st_host[0])
        if bits == 0:
            return out
        if not bits & context.STATUS_F16_RANGE:
            self.nonfinite_pose_forwards += 1
            if self.nonfinite_pose_forwards == 1 and self._f16_pair and pose_of is not None:
                with context.forward(dev, f16_pair=False, force_x3=True, status=None):
                    again = run()
                if bool(torch.isfinite(pose_of(again)).all()):
                    self.logger.error("%s: non-finite pose with NO f16 range bit set, but the fp32x3 re-run is finite: an f16 pair kernel missed its "
                                      "range report (status %d) -- returning the fp32x3 result; set cfg.compute_dtype: fp32x3 and report this", what, bits)
                    return again
                self.logger.warning('%s: non-finite pose (status %d): the fp32x3 re-run is non-finite too -- the inputs or the checkpoint hold NaN / Inf',
                                    what, bits)
            if _throttled(self.nonfinite_pose_forwards):
                self.logger.warning('%s: non-finite pose in the output (status %d; call no. %d with this condition): every f16 pair product was '
                                    'finite, so check the input clouds and the checkpoint for NaN / Inf -- returned as is, not re-run',
                                    what, bits, self.nonfinite_pose_forwards)
            return out
        self.f16_range_fallbacks += 1
        if _throttled(self.f16_range_fallbacks):
            self.logger.warning('%s: f16 pair operand range exceeded (status %d; fallback no. %d) -- re-run with six-term bf16 splits '
                                "(compute_dtype 'fp32x3' arithmetic); set cfg.compute_dtype: fp32x3 to skip the first attempt",
                                what, bits, self.f16_range_fallbacks)
        with context.forward(dev, f16_pair=False, force_x3=True, status=None):
            return run()

    def _needs_pe(self):
        return bool(self.cfg.transformer_encoder_has_pos_emb) or isinstance(self.correspondence_decoder, CorrespondenceDecoder)

    @torch.no_grad()
    def encode_clouds(self, clouds):
        """Everything forward computes of a cloud before it meets a partner, for any number of clouds (nothing is paired, the count
        need not be even): -> regtr_amd.CloudBank with the coarsest key points, feat_proj's output and (when the cross-encoder or the
        attention-valued head reads one) the positional embedding of every cloud, in the order given.  clouds: a list of (n, 3) float32
        GPU tensors.  Runs forward's own code -- _backbone (the two-stream path and the capacity-overflow rebuild included; parity mode
        cfg.kpconv_ref_row_order as it is), the feat_proj GEMM on the prepared weight, pos_embed -- under forward's arithmetic policy
        (_run_checked).  The bank is valid for this model until one of its kpf_encoder / feat_proj / pos_embed weights changes."""
        from .cloud_bank import CloudBank, model_stamp
        clouds = list(clouds)
        if not clouds:
            raise ValueError('RegTR.encode_clouds: no clouds')
        if any(not isinstance(c, torch.Tensor) for c in clouds):
            raise TypeError('RegTR.encode_clouds: clouds must be a list of (n, 3) float32 GPU tensors')
        dev = clouds[0].device
        self._check_placement(dev, clouds, 'encode_clouds')
        stamp = model_stamp(self)

        def run():
            batch = {'src_xyz': clouds, 'tgt_xyz': []}
            feats_un, meta = self._backbone(batch, dev)
            wt = _prepared(self._cache, 'feat_proj', self.feat_proj.weight, lambda w: ops.SplitWeight(w, 'nk'))
            feats = ops.gemm(feats_un, wt, bias=self.feat_proj.bias.detach())
            xyz_c = meta['points'][-1].clone()       # (a row slice of the pyramid's capacity-sized buffer: the bank keeps its own N x 12 bytes)
            pe = self.pos_embed(xyz_c) if self._needs_pe() else None
            return CloudBank(xyz_c, feats, pe, meta['_seg_off'][-1].clone(), meta['_lens_host'][-1], stamp)
        return self._run_checked(dev, run, 'encode_clouds')

    @torch.no_grad()
    def register(self, bank, src_idx, tgt_idx):
        """The P pairs (bank cloud src_idx[k], bank cloud tgt_idx[k]) through everything forward runs after the projection: the
        cross-encoder, the correspondence head and the pose solve -> the dict forward returns for the batch
        {'src_xyz': [cloud src_idx[k]], 'tgt_xyz': [cloud tgt_idx[k]]}, as views of the packed results.  A cloud may appear any number
        of times, on either side; i == j is allowed.  One regtr_gather_segments launch lays the 2P clouds' cached rows out in forward's
        order (sources, then their partners), its tables built from bank.lens on the host and sent in one pinned, non-blocking copy;
        register adds no host wait beyond forward's status read.  A range trip re-runs the call in fp32x3 arithmetic on the SAME bank.
        Refused before any launch: an empty pair list, index lists of different lengths, an index outside the bank, a bank from
        another model, another device or stale weights (CloudBank.check)."""
        from .cloud_bank import CloudBank, upload_tables
        if not isinstance(bank, CloudBank):
            raise TypeError(f'RegTR.register: bank must be a regtr_amd.CloudBank (RegTR.encode_clouds), got {type(bank).__name__}')
        src_idx, tgt_idx = [int(i) for i in src_idx], [int(i) for i in tgt_idx]
        if len(src_idx) != len(tgt_idx):
            raise ValueError(f'RegTR.register: {len(src_idx)} source and {len(tgt_idx)} target indices')
        P = len(src_idx)
        if P == 0:
            raise ValueError('RegTR.register: no pairs')
        bad = [i for i in src_idx + tgt_idx if not 0 <= i < len(bank)]
        if bad:
            raise IndexError(f'RegTR.register: cloud {bad[0]} is not in a bank of {len(bank)}')
        dev = bank.device
        self._check_placement(dev, (bank.feats,), 'register')
        bank.check(self, 'RegTR.register')
        if self._needs_pe() and bank.pe is None:
            raise RuntimeError('RegTR.register: the bank carries no positional embedding but this model reads one')
        order = src_idx + tgt_idx
        lens = [bank.lens[c] for c in order]

        def run():
            seg_c, cloud_of, N, max_len = upload_tables(bank.lens, order, dev)
            both_feats_un, pe_c, xyz_c = ops.gather_segments(bank.feats, bank.seg_off, cloud_of, seg_c, N, max_len, pe=bank.pe, xyz=bank.xyz)
            pe = pe_c if self.cfg.transformer_encoder_has_pos_emb else None
            kv_self, kv_cross = self._kv_tables(P, dev)
            feats_cond = self.transformer_encoder(both_feats_un, pe, seg_c, kv_self, kv_cross, max_len)
            if isinstance(self.correspondence_decoder, CorrespondenceRegressor):
                corr, logit = self.correspondence_decoder(feats_cond)
            else:
                corr, logit = self.correspondence_decoder(feats_cond, pe_c, xyz_c, seg_c, kv_cross, max_len)
            pose = ops.weighted_procrustes(xyz_c, corr, logit, seg_c, P)
            return both_feats_un, feats_cond, xyz_c, corr, logit, pose
        both_feats_un, feats_cond, xyz_c, corr, logit, pose = self._run_checked(dev, run, 'register', pose_of=lambda r: r[-1])
        off = [0]
        for n in lens:
            off.append(off[-1] + n)
        sl = lambda c: slice(off[c], off[c + 1])
        logit3 = logit.unsqueeze(-1)
        return {
            'src_feat_un': tuple(both_feats_un[sl(b)] for b in range(P)),
            'tgt_feat_un': tuple(both_feats_un[sl(P + b)] for b in range(P)),
            'src_feat': [feats_cond[:, sl(b)] for b in range(P)],
            'tgt_feat': [feats_cond[:, sl(P + b)] for b in range(P)],
            'src_kp': tuple(xyz_c[sl(b)] for b in range(P)),
            'src_kp_warped': [corr[:, sl(b)] for b in range(P)],
            'tgt_kp': tuple(xyz_c[sl(P + b)] for b in range(P)),
            'tgt_kp_warped': [corr[:, sl(P + b)] for b in range(P)],
            'src_overlap': [logit3[:, sl(b)] for b in range(P)],
            'tgt_overlap': [logit3[:, sl(P + b)] for b in range(P)],
            'pose': pose,
        }

    # ------------------------------------------------------------------------------------------ training above a frozen backbone
    def _check_trainable(self, what):
        """Everything the differentiable path refuses, before any launch."""
        if not isinstance(self.correspondence_decoder, CorrespondenceRegressor):
            raise NotImplementedError(f'{what}: the attention-valued head (direct_regress_coor: false) has no backward; only '
                                      'CorrespondenceRegressor configs can be trained')
        missing = [k for k in ('r_p', 'r_n', 'wt_overlap', 'wt_feature', 'wt_feature_un', 'wt_corr') if k not in self.cfg]
        if missing:
            raise KeyError(f'{what} needs the losses section of the config (regtr_amd/conf/*.yaml); missing: {missing}')

    def head_layers(self):
        """The decoder layers a loss reads the head's outputs of: cfg.overlap_loss_on | cfg.corr_loss_on, ascending; with the pose term
        on (cfg.wt_pose > 0) always the last layer as well, whose pose it reads."""
        layers = set(self.cfg.overlap_loss_on) | set(self.cfg.corr_loss_on)
        if pose_loss_on(self.cfg):
            layers.add(self.cfg.num_encoder_layers - 1)
        return sorted(layers)

    def forward_grad(self, batch, backbone_grad=False, train_backbone=False):
        """forward(batch) as a differentiable call, by default above a FROZEN backbone: the preprocessor and kpf_encoder run under torch.no_grad()
        as in forward; feat_proj, the cross-encoder and the correspondence head run through head_grad.stack_forward_grad with a HIP
        backward, the head on the decoder layers of head_layers() only.  The arithmetic is that of forward's range fallback
        (compute_dtype 'fp32x3': six-term bf16 splits, float32's operand range), so there is no status word, no end-of-forward wait
        and no re-run.  Returns the reference's dict as forward does, every entry forward also computes bit-identical to it under
        that arithmetic, with two differences:
          * '*_kp_warped' / '*_overlap': per pair a dict {decoder layer: (n, 3) / (n, 1)} over head_layers() -- indexed [b][i] like
            forward's (L, n, .) tensors, the layers no loss reads absent;
          * 'pose': (1, B, 3, 4), the LAST decoder layer's, through head_grad.procrustes_forward_grad: the same launch and bits as
            forward's, with a gradient to that layer's warped points and overlap logits (regtr_weighted_procrustes_bwd, launched only
            when a loss reads the pose; the reference's own loss never does).  Absent when the last layer is not in head_layers().
        backbone_grad=True: feats_un, the backbone's output, becomes a leaf that requires grad and is returned as pred['_feats_un'];
        its .grad after backward() is what a backbone backward starts from.
        train_backbone=True: the preprocessor runs without gradient on one stream and the encoder through KPFEncoder.forward_grad
        inside autograd, so backward() also fills the .grad of every kpf_encoder weight; pred['_feats_un'] is then the (non-leaf)
        encoder output.  This pred is NOT bit-identical to the inference forward: KPFEncoder.forward_grad composes the plain operators,
        whose InstanceNorm statistics come from a pass over the stored rows, where the fused inference routes take them from GEMM
        epilogues and input moments -- the two agree within float32 rounding (docs/PARITY.md holds both to the same float64
        restatement; tests/test_gpu_backbone_grads.py holds this pred to the bars forward is held to on the golden)."""
        from . import head_grad
        self._check_trainable('forward_grad')
        dev = batch['src_xyz'][0].device
        if dev.type != 'cuda':
            raise RuntimeError('regtr_amd.RegTR runs on an MI355X (HIP) device only; there is no CPU path')
        bad = [n for n, p in self.named_parameters() if p.dtype != torch.float32 or p.device != dev]
        if bad or any(p.device != dev for p in batch['src_xyz'] + batch['tgt_xyz']):
            raise RuntimeError(f'RegTR.forward_grad: float32 parameters and every input cloud must live on one GPU ({dev}); offending: {bad[:3]}')
        B = len(batch['src_xyz'])
        layers = self.head_layers()
        with context.forward(dev, f16_pair=False, force_x3=True, status=None):
            if train_backbone:
                feats_un, meta = self._backbone(batch, dev, train=True)
            else:
                with torch.no_grad():
                    feats_un, meta = self._backbone(batch, dev)
                if backbone_grad:
                    feats_un = feats_un.detach().requires_grad_()
            slens_c = meta['_lens_host'][-1]
            xyz_c, seg_c = meta['points'][-1], meta['_seg_off'][-1]
            kv_self, kv_cross = self._kv_tables(B, dev)
            both_feats_un, feats_cond, corr, logit = head_grad.stack_forward_grad(
                self.feat_proj, self.pos_embed if self.cfg.transformer_encoder_has_pos_emb else None, self.transformer_encoder,
                self.correspondence_decoder, feats_un, xyz_c, seg_c, kv_self, kv_cross, max(slens_c), layers, cache=self._cache)
            pose = None
            if layers[-1] == self.cfg.num_encoder_layers - 1:
                pose = head_grad.procrustes_forward_grad(xyz_c, corr[-1:], logit[-1:], seg_c, B).as_subclass(head_grad.PoseTensor)
        off = [0]
        for n in slens_c:
            off.append(off[-1] + n)
        sl = lambda c: slice(off[c], off[c + 1])
        logit3 = logit.unsqueeze(-1)
        per_layer = lambda t, c: {l: t[j, sl(c)] for j, l in enumerate(layers)}
        pred = {
            'src_feat_un': tuple(both_feats_un[sl(b)] for b in range(B)),
            'tgt_feat_un': tuple(both_feats_un[sl(B + b)] for b in range(B)),
            'src_feat': [feats_cond[:, sl(b)] for b in range(B)],
            'tgt_feat': [feats_cond[:, sl(B + b)] for b in range(B)],
            'src_kp': tuple(xyz_c[sl(b)] for b in range(B)),
            'src_kp_warped': [per_layer(corr, b) for b in range(B)],
            'tgt_kp': tuple(xyz_c[sl(B + b)] for b in range(B)),
            'tgt_kp_warped': [per_layer(corr, B + b) for b in range(B)],
            'src_overlap': [per_layer(logit3, b) for b in range(B)],
            'tgt_overlap': [per_layer(logit3, B + b) for b in range(B)],
        }
        if pose is not None:
            pred['pose'] = pose
        if backbone_grad or train_backbone:
            pred['_feats_un'] = feats_un
        return pred

    def compute_loss_grad(self, pred, batch):
        """compute_loss(pred, batch) -- the same keys and reference semantics (regtr.py:237-294) -- as differentiable 0-dim tensors, built
        from the training criteria of regtr_amd/losses.py: the overlap terms on OverlapCriterion's Function (bit-equal to compute_loss's),
        the feature terms on InfoNCELossFull's with this model's feature_criterion.W / feature_criterion_un.W (or on CircleLossFull's
        under feature_loss_type 'circle', with the shared criterion's margins and radii), the correspondence terms
        on CorrCriterion's in both directions (the inverse GT pose for tgt), under cfg.wt_pose > 0 the opt-in pose term
        losses.PoseCriterion on pred['pose'] (a few torch ops; its gradient reaches the head through regtr_weighted_procrustes_bwd),
        the total weighted by loss_weight_dict(cfg).  Gradients go
        to the features, the warped points, the overlap logits and the two W.  No host wait, forward or backward."""
        from . import losses as L
        self._check_trainable('compute_loss_grad')
        cfg = self.cfg
        meta = batch['kpconv_meta']
        B = len(pred['src_kp'])
        dev = pred['src_kp'][0].device
        lens = [int(n) for n in meta['_lens_host'][-1]]
        N, n_src = sum(lens), sum(lens[:B])
        seg_c = meta['_seg_off'][-1]
        wd = loss_weight_dict(cfg)
        def rows(key, i=None):
            """pred's per-pair views of one quantity as ONE packed tensor (src clouds, then tgt clouds).  With a gradient to carry they are
            concatenated (autograd splits it back); _packed_rows' zero-copy view is a function of its first view only."""
            views = [x if i is None else x[i] for x in list(pred['src_' + key]) + list(pred['tgt_' + key])]
            return torch.cat(views, dim=0) if any(v.requires_grad for v in views) else _packed_rows(views)
        with torch.no_grad(), context.forward(dev, f16_pair=False, status=None):
            pose = batch['pose']
            if isinstance(pose, (list, tuple)):
                pose = torch.stack(list(pose))
            pose = pose.to(device=dev, dtype=torch.float32).contiguous()
            batch['overlap_pyr'] = overlap.compute_overlaps(batch)                               # :242-245
            gt_c = batch['overlap_pyr'][f'pyr_{len(meta["points"]) - 1}']
            xyz = rows('kp')
            # T^-1 = [R^T | -R^T t], rounded per operation in regtr_loss_terms' order
            R, t = pose[:, :3, :3], pose[:, :3, 3]
            ti = -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])
            pose_inv = torch.cat([R.transpose(1, 2), ti.unsqueeze(-1)], dim=2).contiguous()
            # the segment tables of the criteria's Functions, derived on the device (regtr_loss_terms' layout with empty tgt clouds)
            seg_s = seg_c[:B + 1]
            seg_t = seg_c[B:] - seg_c[B]
            seg2_s = torch.cat([seg_s, seg_s[-1:].expand(B)])
            seg2_t = torch.cat([seg_t, seg_t[-1:].expand(B)])
            anc_xyz = ops.se3_transform(xyz[:n_src], seg_s, pose)                                 # :259 se3_transform_list(pose_gt, src_kp)
        losses = {}
        for i in cfg.overlap_loss_on:                                                             # :249-252
            warped = rows('kp_warped', i)
            losses[f'overlap_{i}'] = L.overlap_bce(rows('overlap', i).reshape(N), gt_c, seg_c, xyz, warped.detach().contiguous(), pose)
        feat_sets = [(f'feature_{i}', self.feature_criterion, rows('feat', i)) for i in cfg.feature_loss_on]
        feat_sets.append(('feature_un', self.feature_criterion_un, rows('feat_un')))
        circle = isinstance(self.feature_criterion, L.CircleLossFull)
        for key, crit, feats in feat_sets:                                                        # :255-265
            if circle:
                losses[key] = L._Circle.apply(feats[:n_src].contiguous(), feats[n_src:].contiguous(), anc_xyz, xyz[n_src:], seg_s, seg_t,
                                              max(lens[:B]), max(lens[B:]), float(crit.r_p), float(crit.r_n), crit.params())
            else:
                losses[key] = L._InfoNCE.apply(feats[:n_src], feats[n_src:], crit.W, anc_xyz, xyz[n_src:], seg_s, seg_t, max(lens[:B]),
                                               max(lens[B:]), float(cfg.r_p), float(cfg.r_n))
        for i in cfg.corr_loss_on:                                                                # :268-281
            warped = rows('kp_warped', i)
            losses[f'corr_{i}'] = (L._CorrL1.apply(warped[:n_src], xyz[:n_src], gt_c[:n_src], seg_s, seg2_s, pose) +
                                   L._CorrL1.apply(warped[n_src:], xyz[n_src:], gt_c[n_src:], seg_t, seg2_t, pose_inv))
        if pose_loss_on(cfg):                                                                     # opt-in, not a reference loss
            losses[f'pose_{cfg.num_encoder_layers - 1}'] = L.PoseCriterion()(pred['pose'][-1], pose)
        losses['total'] = torch.sum(torch.stack([losses[k] * wd[k] for k in losses]), dim=0)     # :292-293
        return losses

    def trainable_parameters(self, backbone=False):
        """The parameters above the backbone -- feat_proj, the learned positional embedding's ten tensors (pos_emb_type 'learned'; the
        sine embedding has none), the cross-encoder, the correspondence head and the two InfoNCE W -- as a
        list.  Turns requires_grad on for the two W (they are created frozen, which inference keeps; a circle config has none).  backbone=True: kpf_encoder's
        weights as well (what training_step(train_backbone=True) fills); the kernel_points stay requires_grad=False and are not
        listed."""
        mods = [self.feat_proj, self.pos_embed, self.transformer_encoder, self.correspondence_decoder, self.feature_criterion,
                self.feature_criterion_un]
        for crit in mods[4:]:
            if hasattr(crit, 'W'):                    # (CircleLossFull has no parameters)
                crit.W.requires_grad_(True)
        params = [p for m in mods for p in m.parameters()]
        if backbone:
            params += [p for p in self.kpf_encoder.parameters() if p.requires_grad]
        return params

    def configure_optimizers(self, train_backbone=True):
        """generic_reg_model.py:28-62: sets self.optimizer and self.scheduler from cfg.optimizer ('AdamW' | 'Adam'), cfg.base_lr,
        cfg.weight_decay, cfg.grad_clip and cfg.scheduler ('step': StepLR(*cfg.scheduler_param); 'none' / absent: StepLR(50, 1.0);
        'warmup' is not implemented: no shipped config uses it).  The optimiser is regtr_amd.optim.FusedAdamW over
        list(self.parameters()) in that order -- the reference builds its own over self.parameters() too, so the indices of the
        optimiser's state_dict are the reference's; the frozen kernel_points (and, with train_backbone=False, the backbone's weights)
        sit in the list and never get a gradient, hence no state.  The reference's clip_grad_norm_(model.parameters(), cfg.grad_clip)
        lives in the optimiser (max_grad_norm), so a step is: optimizer.zero_grad(), training_step(batch,
        train_backbone=train_backbone), losses['total'].backward(), optimizer.step(), scheduler.step().  cfg.skip_nonfinite (absent:
        off): FusedAdamW(skip_nonfinite=True), which leaves a step with a non-finite gradient out on the device."""
        from .optim import FusedAdamW
        cfg = self.cfg
        scheduler_type = cfg.get('scheduler', None)
        if scheduler_type == 'warmup':
            raise NotImplementedError("scheduler 'warmup' is not implemented (no shipped config uses it)")
        if scheduler_type not in (None, 'none', 'step'):
            raise NotImplementedError(f'scheduler {scheduler_type!r}')
        if cfg.optimizer not in ('AdamW', 'Adam'):
            raise NotImplementedError(f'optimizer {cfg.optimizer!r}: choose AdamW or Adam')
        self.trainable_parameters(backbone=train_backbone)          # turns requires_grad on for the two InfoNCE W
        self.optimizer = FusedAdamW(list(self.parameters()), lr=cfg.base_lr, weight_decay=cfg.weight_decay,
                                    max_grad_norm=cfg.get('grad_clip', 0.0), decoupled=cfg.optimizer == 'AdamW',
                                    **({'skip_nonfinite': True} if cfg.get('skip_nonfinite', False) else {}))
        if scheduler_type == 'step':
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, cfg.scheduler_param[0], cfg.scheduler_param[1])
        else:
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, 50, 1.0)
        self.logger.info(f'Using optimizer {self.optimizer} with scheduler {self.scheduler}')
        return self.optimizer, self.scheduler

    def training_step(self, batch, batch_idx=None, train_backbone=False):
        """generic_reg_model.py:64-66 of the reference: pred = forward_grad(batch), losses = compute_loss_grad(pred, batch) ->
        (pred, losses); the caller runs losses['total'].backward() and steps its optimiser (configure_optimizers).  By default
        the backbone is frozen: kpf_encoder's parameters end with grad None.  train_backbone=True trains it too (forward_grad's
        train_backbone)."""
        pred = self.forward_grad(batch, train_backbone=train_backbone)
        return pred, self.compute_loss_grad(pred, batch)

    # ------------------------------------------------------------------------------------------ losses (validation / test, no gradients)
    def _w_sym(self, crit):
        """InfoNCELossFull's W_sym = triu(W) + triu(W)^T (feature_loss.py:295-296; the diagonal counts twice), once per weight version."""
        return _prepared(self._cache, ('w_sym', id(crit)), crit.W, lambda w: (torch.triu(w) + torch.triu(w).t()).contiguous())

    def _infonce(self, crit, feats, xyz, seg_c, lens, B, pose12, r_p, r_n):
        """Per-pair (masked loss sum, mask count) of InfoNCELossFull.forward on packed tokens (src clouds, then tgt clouds):
        anchors = the src tokens with the GT pose applied to their coordinates, positives = the tgt tokens."""
        n_src = sum(lens[:B])
        pos_t = torch.empty_like(feats)                 # rows [n_src, N) get G W_sym; the src rows are never read
        ops.gemm(feats[n_src:], self._w_sym(crit), out=pos_t[n_src:])                         # exact-f32 MFMA GEMM
        return ops.infonce(feats, pos_t, xyz, xyz, seg_c[:B + 1], seg_c[B:], max(lens[:B], default=0), r_p, r_n, anc_pose=pose12)

    def _circle(self, crit, feats, xyz, seg_c, lens, B, pose12):
        """Per-pair (row-loss sum, selected rows, column-loss sum, selected columns) of CircleLossFull.forward on packed tokens (src
        clouds, then tgt clouds), anchors and positives as in _infonce: regtr_circle_rows reads both sides in place."""
        return ops.circle_rows(feats, feats, xyz, xyz, seg_c[:B + 1], seg_c[B:], max(lens[:B], default=0), max(lens[B:], default=0),
                               float(crit.r_p), float(crit.r_n), crit.params(), anc_pose=pose12)[0]

    def loss_keys(self):
        """The keys of compute_loss's result, in its order."""
        cfg = self.cfg
        return ([f'overlap_{i}' for i in cfg.overlap_loss_on] + [f'feature_{i}' for i in cfg.feature_loss_on] + ['feature_un'] +
                [f'corr_{i}' for i in cfg.corr_loss_on] + ([f'pose_{cfg.num_encoder_layers - 1}'] if pose_loss_on(cfg) else []) + ['total'])

    @torch.no_grad()
    def compute_loss(self, pred, batch, per_pair=False):
        """regtr.py:237-294 without gradients: {'overlap_i', 'feature_i', 'feature_un', 'corr_i', 'total'} (and 'pose_{L-1}', this
        project's opt-in pose term, under cfg.wt_pose > 0: losses.PoseCriterion on pred['pose'][-1]) -> 0-dim device tensors,
        or (B,) tensors of every term per pair with per_pair=True (what the reference computes with one pair per batch).
        batch: 'pose' (B, 3, 4) or (B, 4, 4), 'src_overlap' / 'tgt_overlap' level-0 masks, 'kpconv_meta' from the preceding forward
        (batch['overlap_pyr'] is set as the reference does).  Reference semantics kept, NaN included: a pair without an anchor inside
        r_p gives 0 / 0 in its feature term, and the total is then NaN.  Float32-grade whatever cfg.compute_dtype; no host wait.
        Under feature_loss_type 'circle' a prediction with no pairs raises NotImplementedError (the loss divides by their number)."""
        cfg = self.cfg
        missing = [k for k in ('r_p', 'r_n', 'wt_overlap', 'wt_feature', 'wt_feature_un', 'wt_corr') if k not in cfg]
        if missing:
            raise KeyError(f'compute_loss needs the losses section of the config (regtr_amd/conf/*.yaml); missing: {missing}')
        if cfg.get('feature_loss_type', 'infonce') == 'circle' and len(pred['src_kp']) == 0:
            # CircleLossFull divides by the number of pairs (feature_loss.py:243): there is no circle loss of no pairs, and
            # regtr_circle_rows has no pair to reduce
            raise NotImplementedError("compute_loss: feature_loss_type 'circle' over an empty batch (no pairs) is not implemented")
        meta = batch['kpconv_meta']
        B = len(pred['src_kp'])
        dev = pred['src_kp'][0].device
        lens = [int(n) for n in meta['_lens_host'][-1]]
        N = sum(lens)
        seg_c = meta['_seg_off'][-1]
        wd = loss_weight_dict(cfg)
        with context.forward(dev, f16_pair=False, status=None):
            pose = batch['pose']
            if isinstance(pose, (list, tuple)):
                pose = torch.stack(list(pose))
            pose = pose.to(device=dev, dtype=torch.float32).contiguous()
            pose12 = pose[:, :3, :].reshape(B, 12).contiguous()
            batch['overlap_pyr'] = overlap.compute_overlaps(batch)                               # :242-245
            gt_c = batch['overlap_pyr'][f'pyr_{len(meta["points"]) - 1}']
            xyz = _packed_rows(list(pred['src_kp']) + list(pred['tgt_kp']))
            terms = {}
            for i in sorted(set(cfg.overlap_loss_on) | set(cfg.corr_loss_on)):
                logit = _packed_rows([o[i] for o in pred['src_overlap']] + [o[i] for o in pred['tgt_overlap']]).reshape(N)
                warped = _packed_rows([w[i] for w in pred['src_kp_warped']] + [w[i] for w in pred['tgt_kp_warped']])
                terms[i] = ops.loss_terms(logit.contiguous(), gt_c, xyz, warped.contiguous(), seg_c, pose)
            n_pair = torch.tensor([lens[b] + lens[B + b] for b in range(B)], dtype=torch.float32).to(dev, non_blocking=True) \
                if per_pair else None
            losses = {}
            for i in cfg.overlap_loss_on:                                                         # :252-255 (one mean over all points)
                t = terms[i][:, 0]
                losses[f'overlap_{i}'] = t / n_pair if per_pair else t.sum() / N
            feat_sets = [(f'feature_{i}', self.feature_criterion,
                          _packed_rows([f[i] for f in pred['src_feat']] + [f[i] for f in pred['tgt_feat']])) for i in cfg.feature_loss_on]
            feat_sets.append(('feature_un', self.feature_criterion_un, _packed_rows(list(pred['src_feat_un']) + list(pred['tgt_feat_un']))))
            circle = cfg.get('feature_loss_type', 'infonce') == 'circle'
            for key, crit, feats in feat_sets:                                                    # :258-269, feature_loss.py:303-314
                if circle:                                                                        # feature_loss.py:229-243
                    out = self._circle(crit, feats, xyz, seg_c, lens, B, pose12)
                    per = (out[:, 0] / out[:, 1] + out[:, 2] / out[:, 3]) / 2
                else:
                    out = self._infonce(crit, feats, xyz, seg_c, lens, B, pose12, cfg.r_p, cfg.r_n)
                    per = out[:, 0] / out[:, 1]
                losses[key] = per if per_pair else per.mean()
            for i in cfg.corr_loss_on:                                                            # :271-285, corr_loss.py:18-40
                t = terms[i]
                if per_pair:
                    losses[f'corr_{i}'] = t[:, 1] / t[:, 2].clamp_min(1e-6) + t[:, 3] / t[:, 4].clamp_min(1e-6)
                else:
                    s = t.sum(0)
                    losses[f'corr_{i}'] = s[1] / s[2].clamp_min(1e-6) + s[3] / s[4].clamp_min(1e-6)
            if pose_loss_on(cfg):                                                                 # opt-in, not a reference loss
                from .losses import PoseCriterion
                losses[f'pose_{cfg.num_encoder_layers - 1}'] = PoseCriterion()(pred['pose'][-1], pose, per_pair=per_pair)
            losses['total'] = torch.sum(torch.stack([losses[k] * wd[k] for k in losses]), dim=0)   # :292-293
        return losses

    # ------------------------------------------------------------------------------------------ validation / test (no gradients)
    @torch.no_grad()
    def compute_metrics(self, pred, batch):
        """generic_reg_model.py:197-209 (_compute_metrics for the `pose` key): se3_compare of every decoder layer's pose with the
        ground truth -> {'rot_err_deg', 'trans_err'}, (L, B) float32 device tensors (regtr_pose_metrics, computed in float64).
        `trans_err` is || t_p - R_p R_g^T t_g ||, the reference's (docs/PARITY.md).  No host wait."""
        from . import metrics
        err, _ = metrics.pose_errors(pred['pose'], batch['pose'])
        return {'rot_err_deg': err['rot_err_deg'].to(torch.float32), 'trans_err': err['trans_err'].to(torch.float32)}

    @torch.no_grad()
    def refine_pose(self, batch, pose, max_dist=None, iters=30, method='point_to_point', normal_radius=None):
        """Polishes `pose` ((B, 3, 4) or (B, 4, 4), e.g. forward's pred['pose'][-1]) on the batch's full-resolution clouds
        batch['src_xyz'] / batch['tgt_xyz'] by ICP (regtr_amd/refine.py: icp; no reference counterpart).  max_dist: the correspondence
        distance, by default twice the first subsampling cell.  method: 'point_to_point' (default) or 'point_to_plane', which estimates
        the targets' normals with normal_radius (default twice the first subsampling cell).  Returns refine.ICPResult (pose, fitness,
        inlier_rmse, n_inliers, iters_run), device tensors; enqueued on the current stream, no host wait."""
        from . import refine
        if max_dist is None:
            max_dist = 2 * self.cfg.first_subsampling_dl
        if method == 'point_to_point' and normal_radius is None:
            return refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, max_dist, iters=iters)
        if normal_radius is None:
            normal_radius = 2 * self.cfg.first_subsampling_dl
        return refine.icp(batch['src_xyz'], batch['tgt_xyz'], pose, max_dist, iters=iters, method=method, normal_radius=normal_radius)

    def validation_step(self, batch, batch_idx=None):
        """generic_reg_model.py:82-91: forward (no gradients), compute_loss, compute_metrics -> (losses, metrics).  Reads no parameter's
        .grad and writes none; the only host wait is the forward's status read."""
        pred = self.forward(batch)
        return self.compute_loss(pred, batch), self.compute_metrics(pred, batch)

    @torch.no_grad()
    def validation_epoch_end(self, outputs):
        """generic_reg_model.py:93-104: outputs a list of validation_step results -> (score, {'losses': the mean of every loss key over
        the steps, 'metrics': metrics.aggregate(...)}) with score = reg_success_final as a Python float -- the one host read."""
        from . import metrics
        losses = [o[0] for o in outputs]
        avg_losses = {k: torch.mean(torch.stack([l[k] for l in losses])) for k in losses[0]}
        # (the shipped regtr_amd/conf/*.yaml carry no validation section: the reference configs' 10 degrees / 0.1, as test.py assumes)
        avg_metrics = metrics.aggregate([o[1] for o in outputs], self.cfg.get('reg_success_thresh_rot', 10),
                                        self.cfg.get('reg_success_thresh_trans', 0.1))
        return avg_metrics['reg_success_final'].item(), {'losses': avg_losses, 'metrics': avg_metrics}

    def test_step(self, batch, batch_idx=None):
        """generic_reg_model.py:130-158 without the file output: validation_step's (losses, metrics); under cfg.dataset 'modelnet' with
        batch['tgt_raw'] present, metrics['modelnet'] = metrics.modelnet_metrics(pred['pose'][-1], batch) (the RPMNet / DCP metrics)."""
        from . import metrics
        pred = self.forward(batch)
        out = self.compute_metrics(pred, batch)
        if self.cfg.get('dataset', None) == 'modelnet' and 'tgt_raw' in batch:
            out['modelnet'] = metrics.modelnet_metrics(pred['pose'][-1], batch)
        return self.compute_loss(pred, batch), out
