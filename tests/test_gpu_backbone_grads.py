"""GPU: the differentiable KPConv blocks and encoder (regtr_amd/encoder_grad.py), RegTR.training_step(train_backbone=True) and the fused
max-pool forward (ops.maxpool_fwd_argmax) -- against the float64 restatement tests/backbone_grads_ref.py given the forward's own
LeakyReLU sides, pool winners and neighbour-count flags (from `taps`), and against the stored float64 results of the reference's own
KPFEncoder (tests/golden/backbone_grads_crop_b2.npz, tools/make_golden_backbone_grads.py).

Bars.  Every gradient tensor and every output: max err <= 1e-4 max |ref| (the project's flat bar).  Block and encoder outputs: bit-equal
to the same ops.* calls made without autograd, and between two runs.  The model: the pose / correspondence bars of
tests/test_gpu_model.py on the same golden, losses within 1e-4 relative of compute_loss.  The fused pool: bit-equal to the two launches.

Worst figures measured on an MI355X (printed by the tests, recorded in docs/PARITY.md): see that file.
"""
import numpy as np
import pytest
import torch

from tests import backbone_grads_ref as BR
from tests import norm_pool_grads_ref as NR
from tests.util import gold, load_cfg, seeded_sd

pytestmark = pytest.mark.gpu

FLAT = 1e-4
CASE = '3dmatch_crop_b2'


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device='cuda', dtype=dtype)


def _flat(got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300) if ref.size else 0.0


def _meta_dev(meta):
    """The restatement's host meta as the kpconv_meta fields the blocks read."""
    opt = lambda t: None if t is None else _dev(t, torch.int32)
    seg = [_dev(np.concatenate([[0], np.cumsum(l)]), torch.int32) for l in meta['lens']]
    return {'points': [_dev(p) for p in meta['points']], '_neighbors_i32': [opt(t) for t in meta['neighbors']],
            '_pools_i32': [opt(t) for t in meta['pools']], '_pool_width': list(meta['pool_width']), '_seg_off': seg,
            '_lens_host': [list(l) for l in meta['lens']]}


def _module(blk, c):
    from regtr_amd import kpconv as K
    cfg = load_cfg('3dmatch')
    if blk['kind'] == 'unary':
        m = K.UnaryBlock(c['Cin'], c['Cout'], True, 0.02, no_relu=blk['no_relu'])
    elif blk['kind'] == 'simple':
        m = K.SimpleBlock('simple', c['Cin'], 2 * c['Cout'], c['radius'], 0, cfg)
    else:
        m = K.ResnetBottleneckBlock('resnetb_strided' if blk['strided'] else 'resnetb', c['Cin'], c['Cout'], c['radius'], 0, cfg)
    sd = {k: torch.from_numpy(blk[k]) for k in BR.WEIGHT_NAMES if k in blk}
    if 'kp' in blk:
        sd['KPConv.kernel_points'] = torch.from_numpy(blk['kp'])
        m.KPConv.KP_extent = blk['extent']
    m.load_state_dict(sd, strict=True)
    return m.cuda()


# ---- the same plain ops, called without autograd
def _lin(u, a):
    from regtr_amd import ops
    return ops.gemm(a, ops.SplitWeight(u.mlp.weight.detach(), 'nk'), planes=3)


def _norm(x, seg, max_len, res=None, normed=False, lrelu=True):
    from regtr_amd import ops
    st = ops.instnorm_stats(x, seg, max_len)
    rst = ops.instnorm_stats(res, seg, max_len) if normed else None
    return ops.instnorm_apply(x, seg, max_len, st, res, rst, lrelu=lrelu)


def _plain_block(m, x, meta):
    from regtr_amd import kpconv as K, ops
    if isinstance(m, K.UnaryBlock):
        return _norm(_lin(m, x), meta['_seg_off'][0], max(meta['_lens_host'][0]), lrelu=not m.no_relu)
    v = K._LevelView(meta, m.layer_ind, 'strided' in m.block_name)
    if isinstance(m, K.SimpleBlock):
        return _norm(m.KPConv(v.q_pts, v.s_pts, v.inds, x), v.seg_post, v.max_post)
    f = x
    if isinstance(m.unary1, K.UnaryBlock):
        x = _norm(_lin(m.unary1, f), v.seg_pre, v.max_pre)
    y = _norm(m.KPConv(v.q_pts, v.s_pts, v.inds, x), v.seg_post, v.max_post)
    y2 = _lin(m.unary2, y)
    sc = ops.maxpool(f, v.inds, v.pool_width) if 'strided' in m.block_name else f
    has_sc = isinstance(m.unary_shortcut, K.UnaryBlock)
    if has_sc:
        sc = _lin(m.unary_shortcut, sc)
    return _norm(y2, v.seg_post, v.max_post, res=sc, normed=has_sc)


def _plain_encoder(enc, x, meta):
    for b in enc.encoder_blocks:
        x = _plain_block(b, x, meta)
    return x


def _sides(m, tap, x, meta):
    """The forward's own choices of one block, from its tap: LeakyReLU sides (out > 0), pool winners (ops.maxpool_argmax on the tapped
    input) and the convolution input's row flags (row sum > 0) -> the restatement's `sides` dict."""
    from regtr_amd import kpconv as K, ops
    h = lambda t: t.cpu().numpy()
    s = {'masks': [h(t > 0) for t in tap['norms']], 'winners': [], 'pos': []}
    strided = 'strided' in m.block_name
    inds = meta['_pools_i32' if strided else '_neighbors_i32'][m.layer_ind]
    for p in tap['pools']:
        s['winners'].append(h(ops.maxpool_argmax(p, inds, meta['_pool_width'][m.layer_ind])).astype(np.int64))
    conv_in = tap['norms'][0] if isinstance(m, K.ResnetBottleneckBlock) and isinstance(m.unary1, K.UnaryBlock) else x
    s['pos'].append(h(conv_in.detach().double().sum(1) > 0))
    return s


# ------------------------------------------------------------------------------------------------ 1: the blocks
@pytest.mark.parametrize('name', list(BR.CASES))
def test_block_against_float64(name):
    from regtr_amd import kpconv as K
    blk, meta, x, d_out, c = BR.draw_case(name)
    m, dm = _module(blk, c), _meta_dev(meta)
    need_x = c['Cin'] > 1
    xg = _dev(x).requires_grad_(need_x)

    def run():
        m.zero_grad()
        xg.grad = None
        taps = []
        if blk['kind'] == 'unary':
            out = m.forward_grad(xg, dm['_seg_off'][0], max(dm['_lens_host'][0]))
        else:
            out = m.forward_grad(xg, dm, None, taps)
        (out * _dev(d_out)).sum().backward()
        return out.detach(), taps, {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad}, None if xg.grad is None else xg.grad.clone()
    out, taps, grads, dx = run()
    with torch.no_grad():
        plain = _plain_block(m, xg.detach(), dm)
    assert torch.equal(out, plain), 'forward_grad must be bit-equal to the plain ops without autograd'
    if blk['kind'] == 'unary':
        sides = {'masks': [(out > 0).cpu().numpy()]}
    else:
        assert len(taps) == 1 and len(taps[0]['pools']) == int(blk['strided'])
        sides = _sides(m, taps[0], xg, dm)
    ref = BR.run([blk], x, meta, d_out, sides=[sides], x_grad=need_x, device='cuda')
    worst = {'out': _flat(out, ref['out'])}
    assert set(grads) == {k for (_, k) in ref['grads']} and 'KPConv.kernel_points' not in grads
    for k, g in grads.items():
        worst[k] = _flat(g, ref['grads'][(0, k)])
    if need_x:
        worst['dx'] = _flat(dx, ref['dx'])
    else:
        assert dx is None
    print(f'{name}:', ' '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    assert max(worst.values()) <= FLAT, worst
    if not isinstance(m, K.UnaryBlock):
        assert m.KPConv.kernel_points.grad is None
    out2, _, grads2, dx2 = run()
    assert torch.equal(out, out2) and all(torch.equal(grads[k], grads2[k]) for k in grads) and (dx is None or torch.equal(dx, dx2))


def test_blocks_share_transposed_tables_and_refuse(monkeypatch):
    from regtr_amd import encoder_grad, ops
    blk, meta, x, d_out, c = BR.draw_case('resnetb_strided')
    m, dm = _module(blk, c), _meta_dev(meta)
    tables = encoder_grad.Tables()
    xg = _dev(x).requires_grad_()
    out = m.forward_grad(xg, dm, tables)
    assert len(tables) == 2, 'the pool table at its full width (the convolution) and at pool_width (the pool)'
    out2 = m.forward_grad(xg, dm, tables)
    assert len(tables) == 2 and torch.equal(out.detach(), out2.detach())
    none = encoder_grad.Tables()
    m.forward_grad(_dev(x), dm, none)
    assert len(none) == 1, 'an input without gradient: the pool asks for no table; unary1\'s output still needs the convolution\'s'
    blk, meta, x, d_out, c = BR.draw_case('simple_c1')
    m, dm = _module(blk, c), _meta_dev(meta)
    none = encoder_grad.Tables()
    launches = []
    real = ops.kpconv_gather_bwd
    monkeypatch.setattr(ops, 'kpconv_gather_bwd', lambda *a, **k: launches.append(1) or real(*a, **k))
    m.forward_grad(_dev(x), dm, none).sum().backward()
    assert len(none) == 0 and not launches, 'an input without gradient: no transposed table, nothing launched for dX'
    assert m.KPConv.weights.grad is not None
    xg = _dev(x).requires_grad_()
    m.forward_grad(xg, dm).sum().backward()
    assert len(launches) == 1 and xg.grad is not None, 'the counter sees the dX launch where there is one'
    monkeypatch.setattr(ops, 'kpconv_gather_bwd', real)
    dm['points'][0].requires_grad_()
    with pytest.raises(NotImplementedError):
        m.forward_grad(_dev(x), dm)
    dm['points'][0].requires_grad_(False)
    xg = _dev(x).requires_grad_()
    out = m.forward_grad(xg, dm)
    (gx,) = torch.autograd.grad(out.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()                                                      # double backward


# ------------------------------------------------------------------------------------------------ 2, 4: the encoder and the model
_shared = {}


def _setup():
    """The parity-mode model (the reference's tables, seeded weights, test_gpu_losses' seeded W, wt_feature_un = 0.05 as the frozen
    training-step test sets it), the golden two-pair crop batch, and one encoder run with taps + its float64 restatement."""
    if _shared:
        return _shared
    from regtr_amd import context
    from tests.test_gpu_losses import _golden_batch, _model
    g = gold(f'losses_{CASE}')
    cfg = load_cfg('3dmatch')
    cfg.update({'kpconv_ref_row_order': True})
    cfg.wt_feature_un = 0.05
    model = _model(cfg, g)
    srcs, tgts, extra = _golden_batch(g, CASE)

    def batch():
        b = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
        b.update(extra)
        return b
    dev = torch.device('cuda', torch.cuda.current_device())
    arith = lambda: context.forward(dev, f16_pair=False, force_x3=True, status=None)
    with torch.no_grad(), arith():
        b = batch()
        meta = model.preprocessor(b['src_xyz'] + b['tgt_xyz'])
    enc = model.kpf_encoder
    n0 = meta['points'][0].shape[0]
    ones = torch.ones((n0, 1), device='cuda')
    n_out, c_out = meta['points'][-1].shape[0], enc.encoder_skip_dims[-1]
    d_out = np.random.default_rng(17).normal(0, 1, (n_out, c_out)).astype(np.float32)

    def enc_run(taps):
        model.zero_grad()
        with arith():
            out = enc.forward_grad(ones, meta, taps)
            (out * _dev(d_out)).sum().backward()
        return out.detach(), {k: p.grad.clone() for k, p in enc.named_parameters() if p.grad is not None}
    _shared.update(model=model, batch=batch, cfg=cfg, meta=meta, ones=ones, d_out=d_out, enc_run=enc_run, arith=arith)
    return _shared


def _encoder_reference(s):
    """The float64 restatement of the encoder run with the forward's own sides; computed once."""
    if 'ref' not in s:
        enc, meta = s['model'].kpf_encoder, s['meta']
        taps = []
        out, grads = s['enc_run'](taps)
        sides, cur = [], s['ones']
        for m, tap in zip(enc.encoder_blocks, taps):
            sides.append(_sides(m, tap, cur, meta))
            cur = tap['norms'][-1]
        blocks = BR.encoder_blocks(s['cfg'], {k: v.detach().cpu().numpy() for k, v in s['model'].state_dict().items()})
        s.update(out=out, grads=grads, taps=taps, ref=BR.run(blocks, s['ones'].cpu().numpy(), BR.meta_of(meta), s['d_out'], sides=sides, device='cuda'))
    return s


def test_encoder_against_float64():
    s = _encoder_reference(_setup())
    enc, ref = s['model'].kpf_encoder, s['ref']
    assert len(enc.encoder_blocks) == 11 == len(s['taps'])
    weights = {k for k, p in enc.named_parameters() if p.requires_grad}
    assert set(s['grads']) == weights == {f'encoder_blocks.{i}.{k}' for (i, k) in ref['grads']}, 'every encoder weight is checked'
    worst = ('', 0.0)
    for (i, k), want in ref['grads'].items():
        e = _flat(s['grads'][f'encoder_blocks.{i}.{k}'], want)
        print(f'encoder block {i} {k}: {e:.2e}')
        worst = max(worst, (f'{i}.{k}', e), key=lambda t: t[1])
    e_out = _flat(s['out'], ref['out'])
    with torch.no_grad(), s['arith']():
        fused, _ = enc(s['ones'], s['meta'])
        plain = _plain_encoder(enc, s['ones'], s['meta'])
    print(f'encoder: worst gradient {worst[0]} {worst[1]:.2e}; output forward_grad {e_out:.2e}, fused inference forward (fp32x3) '
          f'{_flat(fused, ref["out"]):.2e} of the float64 restatement')
    assert worst[1] <= FLAT and e_out <= FLAT
    assert torch.equal(s['out'], plain), 'forward_grad must be bit-equal to the plain ops without autograd'
    assert all(b.KPConv.kernel_points.grad is None for b in enc.encoder_blocks)


def test_encoder_is_reproducible_and_taps_change_nothing():
    s = _encoder_reference(_setup())
    out_none, grads_none = s['enc_run'](None)
    out_list, grads_list = s['enc_run']([])
    for out, grads in ((out_none, grads_none), (out_list, grads_list)):
        assert torch.equal(out, s['out']) and set(grads) == set(s['grads'])
        assert all(torch.equal(grads[k], s['grads'][k]) for k in grads)


# ------------------------------------------------------------------------------------------------ 3: against the real reference modules
def test_encoder_against_the_reference_modules():
    """The sampled gradients of the reference's own KPFEncoder, run in float64 on the CPU on a cut-down crop with its own tables
    (tools/make_golden_backbone_grads.py), at 1e-4 of the stored maxima -- after asserting that this forward took the float64 run's
    side of every LeakyReLU and its winner of every pool (else the comparison is void: it is not a tolerance question)."""
    from regtr_amd import RegTR, context, ops
    g = gold('backbone_grads_crop_b2')
    cfg = load_cfg('3dmatch')
    cfg.update({'kpconv_ref_row_order': True})
    model = RegTR(cfg)
    model.load_state_dict(seeded_sd(cfg, int(g['seed'])), strict=True)
    model = model.cuda()
    enc = model.kpf_encoder
    clouds = [torch.from_numpy(g[f'cloud_{i}']).cuda() for i in range(int(g['n_clouds']))]
    dev = clouds[0].device
    taps = []
    with context.forward(dev, f16_pair=False, force_x3=True, status=None):
        with torch.no_grad():
            meta = model.preprocessor(clouds)
        assert [int(p.shape[0]) for p in meta['points']] == list(g['level_sizes']), 'the pyramid is not the reference preprocessor\'s'
        ones = torch.ones((meta['points'][0].shape[0], 1), device='cuda')
        out = enc.forward_grad(ones, meta, taps)
        assert int(g['d_out_seed']) == BR.D_OUT_SEED
        (out * _dev(BR.golden_d_out(tuple(out.shape)))).sum().backward()
    assert float(g['margin']) >= 2.0 ** -19
    # the sides: every LeakyReLU mask and every pool winner of the float64 run, bit-packed / int8 in the golden
    n_mask = n_pool = 0
    for i, (m, tap) in enumerate(zip(enc.encoder_blocks, taps)):
        for j, t in enumerate(tap['norms']):
            want = np.unpackbits(g[f'mask_{i}_{j}'])[:t.numel()].reshape(tuple(t.shape)).astype(bool)
            assert np.array_equal((t > 0).cpu().numpy(), want), f'block {i} LeakyReLU {j}: the float32 forward took another side'
            n_mask += 1
        for t in tap['pools']:
            arg = ops.maxpool_argmax(t, meta['_pools_i32'][m.layer_ind], meta['_pool_width'][m.layer_ind]).cpu().numpy()
            assert np.array_equal(arg, g[f'winner_{i}'].astype(np.int16)), f'block {i}: the float32 forward pooled another winner'
            n_pool += 1
    assert n_mask == int(g['n_masks']) and n_pool == 3
    e_out = _flat(out[::int(g['row_step'])], g['out'])
    worst = ('', 0.0)
    names = [k[2:] for k in g.files if k.startswith('g/')]
    params = dict(enc.named_parameters())
    assert set(names) == {k for k, p in params.items() if p.requires_grad}
    for k in names:
        got = params[k].grad.detach().double().cpu().numpy().reshape(-1)[g['i/' + k].astype(np.int64)]
        e = np.abs(got - g['g/' + k]).max() / float(g['m/' + k])
        print(f'vs the reference KPFEncoder {k}: {e:.2e}')
        worst = max(worst, (k, e), key=lambda t: t[1])
    print(f'vs the reference KPFEncoder: worst gradient {worst[0]} {worst[1]:.2e}, output {e_out:.2e}')
    assert worst[1] <= FLAT and e_out <= FLAT


# ------------------------------------------------------------------------------------------------ 4: the model
def _step(s, train_backbone=True):
    model = s['model']
    for p in model.parameters():
        p.grad = None
    b = s['batch']()
    pred, losses = model.training_step(b, train_backbone=train_backbone) if train_backbone else model.training_step(b)
    losses['total'].backward()
    return b, pred, losses


def test_training_step_trains_the_backbone():
    s = _setup()
    model = s['model']
    above = model.trainable_parameters()
    params = model.trainable_parameters(backbone=True)
    enc_w = [p for k, p in model.kpf_encoder.named_parameters() if not k.endswith('kernel_points')]
    assert len(params) == len(set(map(id, params))) == len(above) + len(enc_w) and {id(p) for p in enc_w} <= {id(p) for p in params}
    assert all(not p.requires_grad for k, p in model.kpf_encoder.named_parameters() if k.endswith('kernel_points'))
    b, pred, losses = _step(s)
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all()
    for k, p in model.kpf_encoder.named_parameters():
        if k.endswith('kernel_points'):
            assert p.grad is None
        else:
            assert p.grad.abs().max() > 0, k
    fu = pred['_feats_un']
    assert not fu.is_leaf and fu.requires_grad
    # pred: the bars tests/test_gpu_model.py holds forward to on this golden (parity mode, the real reference module's outputs)
    g = gold(CASE)
    worst = {}
    for bb in range(2):
        assert np.array_equal(pred['src_kp'][bb].cpu().numpy(), g[f'src_kp_{bb}']) and np.array_equal(pred['tgt_kp'][bb].cpu().numpy(), g[f'tgt_kp_{bb}'])
        for k in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
            worst[k] = max(worst.get(k, 0.0), float(np.abs(pred[k][bb][5].detach().cpu().numpy() - g[f'{k}_{bb}'][5]).max()))
    worst['pose'] = float(np.abs(pred['pose'][0].cpu().numpy() - g['pose'][5]).max())
    print('training_step(train_backbone=True) pred: max abs diff vs the reference module:', {k: f'{v:.2e}' for k, v in worst.items()})
    assert max(worst.values()) < 1e-4, worst
    # losses: compute_loss on the same pred
    ref = model.compute_loss(pred, b)
    assert list(losses) == list(ref) == model.loss_keys()
    for k in ref:
        got, w = float(losses[k]), float(ref[k])
        print(f'training_step(train_backbone=True) {k}: {got:.7f} vs compute_loss {w:.7f}')
        assert np.isfinite(got) and abs(got - w) <= 1e-4 * abs(w), k
    # the default call still freezes the backbone
    _step(s, train_backbone=False)
    assert all(p.grad is None for p in model.kpf_encoder.parameters())
    assert all(p.grad is not None for p in above)


def test_backbone_backward_no_host_sync():
    s = _setup()
    model = s['model']
    _step(s)                                                        # weight preparation (once per weight version)
    b = s['batch']()
    pred, losses = model.training_step(b, train_backbone=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses['total'].backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(torch.isfinite(p.grad).all() for p in model.trainable_parameters(backbone=True))


def test_ten_sgd_steps_over_all_parameters_lower_the_total():
    """Ten plain SGD steps over trainable_parameters(backbone=True) on the one batch, at the frozen ten-step test's step size."""
    from tests.test_gpu_head_grads import SGD_LR
    s = _setup()
    model = s['model']
    params = model.trainable_parameters(backbone=True)
    state = [p.detach().clone() for p in model.parameters()]
    try:
        hist = []
        for _ in range(11):
            _, _, losses = _step(s)
            hist.append(float(losses['total'].detach()))
            with torch.no_grad():
                for p in params:
                    p -= SGD_LR * p.grad
        print('total per step:', ' '.join(f'{h:.5f}' for h in hist))
        assert all(np.isfinite(hist)) and hist[-1] < hist[0]
    finally:
        with torch.no_grad():
            for p, st in zip(model.parameters(), state):
                p.copy_(st)


# ------------------------------------------------------------------------------------------------ 5: the fused pool forward
@pytest.mark.parametrize('name', NR.POOL_CASES)
def test_maxpool_fwd_argmax_equals_the_two_launches(name):
    from regtr_amd import ops
    c = NR.draw_case(name)
    x, nbr = _dev(c['x']), _dev(c['nbr'], torch.int32)
    width = None if c['width'] == c['ld'] else c['width']
    nq, C = c['Nq'], c['C']
    guard_o = torch.full((nq + 2, C), -7.0, device='cuda')
    guard_a = torch.full((nq + 2, C), 77, dtype=torch.int16, device='cuda')
    out, arg = ops.maxpool_fwd_argmax(x, nbr, width, out=guard_o[1:nq + 1], out_arg=guard_a[1:nq + 1])
    want_o, want_a = ops.maxpool(x, nbr, width), ops.maxpool_argmax(x, nbr, width)
    assert torch.equal(out.view(torch.int32), want_o.view(torch.int32)), 'out must be bit-equal to ops.maxpool'
    assert torch.equal(arg, want_a)
    assert torch.all(guard_o[0] == -7.0) and torch.all(guard_o[-1] == -7.0) and torch.all(guard_a[0] == 77) and torch.all(guard_a[-1] == 77)
    ref = NR.pool_run(c['x'], c['nbr'], c['width'], c['dy'])
    assert np.array_equal(arg.cpu().numpy(), ref['arg']) and np.array_equal(out.cpu().numpy().astype(np.float64), ref['out'])
    out2, arg2 = ops.maxpool_fwd_argmax(x, nbr, width)
    assert torch.equal(out2, out) and torch.equal(arg2, arg)


def test_maxpool_fwd_argmax_empty():
    from regtr_amd import ops
    x = torch.randn(10, 64, device='cuda')
    out, arg = ops.maxpool_fwd_argmax(x, torch.zeros((0, 7), dtype=torch.int32, device='cuda'))
    assert out.shape == (0, 64) and arg.shape == (0, 64) and arg.dtype is torch.int16
    nbr = torch.zeros((5, 3), dtype=torch.int32, device='cuda')
    out, arg = ops.maxpool_fwd_argmax(torch.zeros((0, 8), device='cuda'), nbr)              # no supports: the shadow row everywhere
    assert torch.all(out == 0) and torch.all(arg == -1)
