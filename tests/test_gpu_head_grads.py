"""GPU: training above a frozen backbone -- the two new kernels (ops.head_tail_bwd, ops.bce_logits_bwd), CorrespondenceRegressor.forward_grad,
losses.OverlapCriterion, head_grad.stack_forward_grad and RegTR.training_step -- against the float64 restatement
tests/head_grads_ref.py and the stored results of the real reference modules (tests/golden/head_grads_<case>.npz).

Bars.  Kernels: err <= the restatement's per-element bound, and max err <= 1e-4 max |ref| (the flat bar of the loss, attention and
cross-encoder gradients); g2 is exactly +0 where the ReLU cut, r is the correctly rounded product.  Head: every parameter gradient and
d feats at max err <= 1e-4 max |ref|.  Stack: every loss term within 1e-5 relative of the reference modules', every gradient tensor at
max err <= 1e-4 max |ref|; a tensor of the STACK beyond that is held to 4x the error of the restatement itself run in float32 torch on
the same GPU (3x: the header's f16 pair vs bf16x3 figure, + 1 for the longer chain).  training_step: bit-equal to the inference
arithmetic it restates, losses within 1e-6 relative of compute_loss."""
import numpy as np
import pytest
import torch

from tests import head_grads_ref as HR
from tests.util import gold, load_cfg

pytestmark = pytest.mark.gpu

FLAT = 1e-4
ROWS = [0, 1, 3, 4, 5, 257, 4099]
FAKE = 0x10000                      # a 16-byte aligned non-NULL address for calls that must be refused before anything reads it
SGD_LR = 1e-4                       # test_ten_sgd_steps_lower_the_total: see its docstring


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(device='cuda', dtype=dtype)


def _np(t):
    return t.detach().double().cpu().numpy()


def _flat(got, ref):
    ref = np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref, dtype=np.float64)
    return np.abs(_np(got) - ref).max() / max(np.abs(ref).max(), 1e-300)


def _ratio(err, bound):
    """max err / bound; a zero bound (exact zeros) admits a zero error only."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf)).max() if err.size else 0.0


# ------------------------------------------------------------------------------------------------ 1, 2: the kernels
@pytest.mark.parametrize('sides', ['both', 'corr', 'logit'])
@pytest.mark.parametrize('D', [64, 256])
def test_head_tail_bwd_against_float64(D, sides):
    from regtr_amd import ops
    rng = np.random.default_rng(300 + D + len(sides))
    names = ('g2', 'r', 'dw4', 'db4', 'dwc', 'dbc', 'db2')
    for m in ROWS:
        h2 = np.maximum(rng.normal(0, 1, (m, D)), 0).astype(np.float32)              # exact zeros where the ReLU cut
        if m:
            h2[0, :4] = [0.0, -0.0, 1e-30, 1.0]
        f, w4, wc = (rng.normal(0, 1, s).astype(np.float32) for s in ((m, D), (3, D), (D,)))
        dc = rng.normal(0, 1, (m, 3)).astype(np.float32) if sides != 'logit' else None
        dl = rng.normal(0, 1, m).astype(np.float32) if sides != 'corr' else None
        ref = HR.head_tail_bwd(dc, dl, h2, f, w4, wc)
        t = lambda a: None if a is None else _dev(a)
        bufs = [torch.full((m + 2, D), -7.0, device='cuda') for _ in range(2)]
        run = lambda g2, r: ops.head_tail_bwd(t(dc), t(dl), t(h2), t(f), t(w4), t(wc), out_g2=g2, out_r=r)
        got = dict(zip(names, run(bufs[0][:m], bufs[1][:m])))
        assert got['g2'].data_ptr() == bufs[0][:m].data_ptr() and got['r'].data_ptr() == bufs[1][:m].data_ptr()
        assert torch.all(bufs[0][m:] == -7.0) and torch.all(bufs[1][m:] == -7.0), 'rows past m were written'
        # selections and single products are exact
        cut = _dev(h2) <= 0
        assert torch.all(got['g2'][cut] == 0) and not torch.signbit(got['g2'][cut]).any(), 'g2 must be +0 where the ReLU cut'
        assert np.array_equal(got['r'].cpu().numpy(), ref['r32']), 'r is one product: the correctly rounded one'
        for k in names:
            want = ref[k]
            assert tuple(got[k].shape) == want.shape, (k, got[k].shape)
            err = np.abs(_np(got[k]) - want)
            ratio = _ratio(err, ref['b_' + k])
            flat = err.max() / max(np.abs(want).max(), 1e-300) if err.size else 0.0
            print(f'head_tail_bwd m={m} D={D} {sides} {k}: err/bound {ratio:.3f} flat {flat:.2e}')
            assert ratio <= 1.0 and flat <= FLAT, (m, k, ratio, flat)
        again = dict(zip(names, run(None, None)))
        for k in names:
            assert torch.equal(got[k], again[k]), (m, k, 'two runs differ')


def _tail(m=100, D=64, ws_bytes=None, **kw):
    from regtr_amd import _lib
    L = _lib.lib()
    names = ('dcorr', 'dlogit', 'h2', 'f', 'W4', 'wc', 'g2', 'r', 'dW4', 'db4', 'dwc', 'dbc', 'db2', 'ws')
    p = {n: kw.get(n, FAKE + 0x1000 * i) for i, n in enumerate(names)}                # distinct: only the named cases alias
    nb = L.regtr_head_tail_bwd_ws_bytes(m, D) if ws_bytes is None else ws_bytes
    return L.regtr_head_tail_bwd(p['dcorr'], p['dlogit'], p['h2'], p['f'], p['W4'], p['wc'], m, D, p['g2'], p['r'], p['dW4'], p['db4'],
                                 p['dwc'], p['dbc'], p['db2'], p['ws'], nb, None)


@pytest.mark.parametrize('kw', [{'m': -1}, {'D': 0}, {'D': 32}, {'D': 96}, {'D': 100}, {'h2': None}, {'f': None}, {'W4': None}, {'wc': None},
                                {'g2': None}, {'r': None}, {'dW4': None}, {'db4': None}, {'dwc': None}, {'dbc': None}, {'ws': None},
                                {'h2': FAKE + 4}, {'f': FAKE + 8}, {'W4': FAKE + 4}, {'wc': FAKE + 12}, {'g2': FAKE + 4}, {'r': FAKE + 8},
                                {'ws': FAKE + 4}, {'g2': FAKE + 64, 'r': FAKE + 64}, {'g2': FAKE + 64, 'h2': FAKE + 64},
                                {'g2': FAKE + 64, 'f': FAKE + 64}, {'r': FAKE + 64, 'h2': FAKE + 64}, {'r': FAKE + 64, 'f': FAKE + 64}])
def test_head_tail_bwd_refuses_bad_arguments(kw):
    """REGTR_ERR_ARG before any launch: the pointers are never read (they point nowhere)."""
    assert _tail(**kw) == -2, kw


def test_head_tail_bwd_workspace_and_empty():
    from regtr_amd import _lib
    assert _tail(ws_bytes=16) == -3
    assert _tail(m=0) == 0 and _tail(m=0, h2=None, g2=None, ws=None) == 0            # nothing to do: nothing is read
    L = _lib.lib()
    assert L.regtr_bce_logits_bwd(FAKE, FAKE, FAKE, -1, FAKE, None) == -2 and L.regtr_bce_logits_bwd(None, None, None, 0, None, None) == 0
    for bad in range(4):
        p = [FAKE] * 4
        p[bad] = None
        assert L.regtr_bce_logits_bwd(p[0], p[1], p[2], 10, p[3], None) == -2


def _bce_inputs(rng, n):
    x = rng.normal(0, 4, n).astype(np.float32)
    y = rng.uniform(0, 1, n).astype(np.float32)
    for i, (xv, yv) in enumerate(((100.0, 0.0), (-100.0, 1.0), (0.0, 0.5), (100.0, 1.0), (-100.0, 0.0))):
        if i < n:
            x[i], y[i] = xv, yv
    y[n // 2:n // 2 + 2] = [0.0, 1.0][:len(y[n // 2:n // 2 + 2])]
    return x, y


def test_bce_logits_bwd_against_float64():
    from regtr_amd import ops
    rng = np.random.default_rng(400)
    for n in ROWS:
        x, y = _bce_inputs(rng, n)
        for g in (1.0, -0.37):
            got = ops.bce_logits_bwd(_dev(x), _dev(y), torch.tensor(g, device='cuda'))
            assert got.shape == (n,)
            if n == 0:
                continue
            r = HR.bce_logits_bwd(x, y, np.float32(g))
            err = np.abs(_np(got) - r['d'])
            print(f'bce_logits_bwd n={n} g={g}: err/bound {_ratio(err, r["b_d"]):.3f} flat {err.max() / np.abs(r["d"]).max():.2e}')
            assert torch.isfinite(got).all() and _ratio(err, r['b_d']) <= 1.0 and err.max() <= FLAT * np.abs(r['d']).max()


def test_overlap_criterion_is_bce_with_logits():
    from regtr_amd import ops
    from regtr_amd.losses import OverlapCriterion
    rng = np.random.default_rng(401)
    lens = [33, 64, 1, 129]
    n = sum(lens)
    x, y = _bce_inputs(rng, n)
    xr = torch.from_numpy(x).double().requires_grad_()
    want = torch.nn.BCEWithLogitsLoss()(xr, torch.from_numpy(y).double())
    (want * 0.7).backward()
    crit = OverlapCriterion()
    seg = _dev(HR.R.offsets(lens), torch.int32)
    for seg_off in (None, seg):
        xg = _dev(x).requires_grad_()
        loss = crit(xg, _dev(y), seg_off)
        (loss * 0.7).backward()
        assert abs(float(loss) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
        assert _flat(xg.grad, xr.grad) <= FLAT
    # with the pair layout the value is RegTR.compute_loss's overlap term, bit for bit: regtr_loss_terms' per-pair sums, added, over n
    kp = torch.zeros((n, 3), device='cuda')
    pose = torch.eye(3, 4, device='cuda').expand(2, 3, 4).contiguous()
    terms = ops.loss_terms(_dev(x), _dev(y), kp, kp, seg, pose)
    assert torch.equal(loss.detach(), terms[:, 0].sum() / n)
    with pytest.raises(RuntimeError):
        crit(torch.from_numpy(x), torch.from_numpy(y))
    with pytest.raises(RuntimeError):
        crit(_dev(x), _dev(y).requires_grad_())


# ------------------------------------------------------------------------------------------------ 3: the head
def _head(c):
    from regtr_amd.regtr import CorrespondenceRegressor
    head = CorrespondenceRegressor(c['D'])
    head.load_state_dict(c['sd'], strict=True)
    return head.cuda()


def _run_head(c, f16=False):
    from regtr_amd import ops
    head = _head(c)
    feats = _dev(c['feats']).requires_grad_()
    with ops.f16_pair(f16):
        corr, logit = head.forward_grad(feats)
        ((corr * _dev(c['d_corr'])).sum() + (logit * _dev(c['d_logit'])).sum()).backward()
    grads = {k: p.grad for k, p in head.named_parameters()}
    grads['df'] = feats.grad
    return head, corr, logit, grads


@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('name', list(HR.HEAD_CASES))
def test_regressor_forward_grad(name, f16):
    from regtr_amd import head_grad, ops
    c = HR.draw_head_case(name)
    ref = HR.run_head_case(c)
    head, corr, logit, grads = _run_head(c, f16)
    with ops.f16_pair(f16), torch.no_grad():
        want_corr, want_logit = head(_dev(c['feats']))
        ng_corr, ng_logit = head.forward_grad(_dev(c['feats']))
    assert corr.requires_grad and logit.requires_grad and not ng_corr.requires_grad
    assert torch.equal(corr.detach(), want_corr) and torch.equal(logit.detach(), want_logit), 'forward_grad must be bit-identical to forward'
    assert torch.equal(ng_corr, want_corr) and torch.equal(ng_logit, want_logit)
    assert _flat(corr, ref['corr']) <= FLAT and _flat(logit, ref['logit']) <= FLAT
    want = dict(ref['grads'], df=ref['df'])
    assert set(grads) == set(want) and all(g is not None for g in grads.values())
    for k in sorted(want):
        e = _flat(grads[k], want[k])
        print(f'{name} f16_pair={f16} {k}: {e:.2e}')
        assert tuple(grads[k].shape) == tuple(want[k].shape) and e <= FLAT, (k, e)
    # twice the same bits; and the composed tail (the generic ops) computes the same gradients
    _, _, _, again = _run_head(c, f16)
    assert all(torch.equal(grads[k], again[k]) for k in grads)
    saved = head_grad.use_fused_tail
    try:
        head_grad.use_fused_tail = False
        _, _, _, comp = _run_head(c, f16)
    finally:
        head_grad.use_fused_tail = saved
    for k in sorted(want):
        assert _flat(comp[k], want[k]) <= FLAT, ('composed', k)


def test_regressor_one_output_used_and_refusals():
    c = HR.draw_head_case('ragged')
    ref = HR.run_head_case(c)
    head = _head(c)
    feats = _dev(c['feats']).requires_grad_()
    _, logit = head.forward_grad(feats)
    (logit * _dev(c['d_logit'])).sum().backward()                                     # the coordinate MLP took no part
    assert all(p.grad is None for p in head.coor_mlp.parameters())
    assert _flat(head.conf_logits_decoder.weight.grad, ref['grads']['conf_logits_decoder.weight']) <= FLAT
    wc = c['sd']['conf_logits_decoder.weight'].double()
    assert _flat(feats.grad, c['d_logit'].double()[..., None] * wc) <= FLAT
    head.zero_grad()
    feats.grad = None
    corr, _ = head.forward_grad(feats)
    (corr * _dev(c['d_corr'])).sum().backward()
    assert head.conf_logits_decoder.weight.grad is None and _flat(head.coor_mlp[4].weight.grad, ref['grads']['coor_mlp.4.weight']) <= FLAT
    with pytest.raises(RuntimeError):
        head.forward_grad(c['feats'])                                                 # a CPU tensor
    corr, logit = head.forward_grad(feats)
    (gx,) = torch.autograd.grad(corr.sum() + logit.sum(), feats, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()                                                           # double backward


def test_decoder_head_and_its_config_are_refused():
    from regtr_amd import RegTR
    from regtr_amd.regtr import CorrespondenceDecoder
    with pytest.raises(NotImplementedError):
        CorrespondenceDecoder(64, True).forward_grad(torch.zeros(1, 4, 64))
    cfg = load_cfg('3dmatch')
    cfg.direct_regress_coor = False
    model = RegTR(cfg)                                                                # on the CPU: refused before any launch
    with pytest.raises(NotImplementedError):
        model.training_step({'src_xyz': [torch.zeros(4, 3)], 'tgt_xyz': [torch.zeros(4, 3)]})


# ------------------------------------------------------------------------------------------------ 4: the stack against the reference modules
def _stack_run(c):
    """stack_forward_grad + the three criteria on a drawn case, the weighted total, backward -> (losses, corr, logit, grads)."""
    from regtr_amd import head_grad
    from regtr_amd.losses import CorrCriterion, InfoNCELossFull, OverlapCriterion
    from regtr_amd.regtr import CorrespondenceRegressor
    from regtr_amd.transformer import TransformerCrossEncoder, TransformerCrossEncoderLayer
    D, B, L, wt = c['D'], c['B'], c['L'], c['wt']
    feat_proj = torch.nn.Linear(c['K'], D)
    feat_proj.load_state_dict(c['sd_proj'])
    layer = TransformerCrossEncoderLayer(D, c['H'], c['F'], 0.0, 'relu', True, True, True)
    enc = TransformerCrossEncoder(layer, L, torch.nn.LayerNorm(D), return_intermediate=True)
    enc.load_state_dict(c['sd_enc'], strict=True)
    head = CorrespondenceRegressor(D)
    head.load_state_dict(c['sd_head'], strict=True)
    crit, crit_un = InfoNCELossFull(D, c['r_p'], c['r_n']), InfoNCELossFull(D, c['r_p'], c['r_n'])
    with torch.no_grad():
        crit.W.copy_(c['W'])
        crit_un.W.copy_(c['W_un'])
    mods = {'feat_proj': feat_proj, 'transformer_encoder': enc, 'correspondence_decoder': head, 'feature_criterion': crit,
            'feature_criterion_un': crit_un}
    for m in mods.values():
        m.cuda()
    pe = None if c['pe'] is None else _dev(c['pe'])
    feats_un = _dev(c['feats_un']).requires_grad_()
    seg = _dev(c['seg'], torch.int32)
    both, feats_cond, corr, logit = head_grad.stack_forward_grad(
        feat_proj, None if pe is None else (lambda xyz: pe), enc, head, feats_un, _dev(c['xyz']), seg, _dev(c['kv_self'], torch.int32),
        _dev(c['kv_cross'], torch.int32), c['max_len'], [L - 1])
    assert tuple(feats_cond.shape) == (L, len(c['xyz']), D) and tuple(corr.shape) == (1, len(c['xyz']), 3) and tuple(logit.shape) == corr.shape[:2]
    s = c['seg']
    cut = lambda x, lo: [x[int(s[lo + b]):int(s[lo + b + 1])] for b in range(B)]
    gt, pose = _dev(c['gt']), _dev(c['pose'])
    anc, src_kp, tgt_kp = [_dev(a) for a in c['anc']], [_dev(a) for a in c['src_kp']], [_dev(a) for a in c['tgt_kp']]
    last = feats_cond[L - 1]
    corr_crit = CorrCriterion('mae')
    losses = {'overlap': OverlapCriterion()(logit[0], gt, seg),
              'feature': crit(cut(last, 0), cut(last, B), anc, tgt_kp),
              'feature_un': crit_un(cut(both, 0), cut(both, B), anc, tgt_kp),
              'corr': (corr_crit(src_kp, cut(corr[0], 0), pose, cut(gt, 0)) +
                       corr_crit(tgt_kp, cut(corr[0], B), HR.se3_inv(pose).contiguous(), cut(gt, B)))}
    losses['total'] = torch.sum(torch.stack([losses[k] * wt[k] for k in ('overlap', 'feature', 'feature_un', 'corr')]))
    losses['total'].backward()
    grads = {f'{mk}.{k}': p.grad for mk, m in mods.items() for k, p in m.named_parameters()}
    return losses, corr[0], logit[0], feats_un.grad, grads


@pytest.mark.parametrize('name', list(HR.FULL_CASES))
def test_stack_against_the_real_reference_modules(name):
    """stack_forward_grad + OverlapCriterion / InfoNCELossFull / CorrCriterion against the stored float64 results of the reference's own
    modules.  Losses 1e-5 relative; every gradient tensor at 1e-4 max |ref|, beyond that at 4x the error of the restatement run in
    float32 torch on this GPU; no gradient tensor is skipped."""
    c = HR.draw_full_case(name)
    g = gold(f'head_grads_{name}')
    st, rows = int(g['row_step']), g['w_rows']
    losses, corr, logit, d_fu, grads = _stack_run(c)
    for k in ('overlap', 'feature', 'feature_un', 'corr', 'total'):
        got, want = float(losses[k]), float(g['loss/' + k])
        print(f'{name} loss {k}: {got:.7f} vs {want:.7f} ({abs(got - want) / abs(want):.2e})')
        assert abs(got - want) <= 1e-5 * abs(want), k
    assert _flat(corr[::st], g['corr']) <= FLAT and _flat(logit[::st], g['logit']) <= FLAT
    names = [k[2:] for k in g.files if k.startswith('g/')]
    assert set(names) == set(grads) and all(v is not None for v in grads.values()), 'every gradient tensor of the reference is checked'
    sub = lambda t: t if t.dim() == 1 or t.shape[0] <= 3 else t[rows]
    f32, beyond = None, []
    for k, got, want in [('d_feats_un', d_fu[::st], g['d_feats_un'])] + [(k, sub(grads[k]), g['g/' + k]) for k in names]:
        e = _flat(got, want)
        bar = FLAT
        if e > FLAT:
            if f32 is None:
                f32 = HR.full(c, dtype=torch.float32, device='cuda')
            t = f32['d_feats_un'][::st] if k == 'd_feats_un' else sub(f32['grads'][k])
            bar = 4 * _flat(t, want)
        print(f'{name} vs reference {k}: {e:.2e} (bar {bar:.2e})')
        if e > bar:
            beyond.append((k, e, bar))
    assert not beyond, beyond


# ------------------------------------------------------------------------------------------------ 5: RegTR.training_step
CASE = '3dmatch_crop_b2'
_shared = {}


def _setup():
    """The model (seeded weights, test_gpu_losses' seeded W; feature_un given a weight so that its W takes a gradient: the shipped 0.0
    makes that gradient vanish by construction), the golden batch, and the first training step's (pred, losses) before backward."""
    if not _shared:
        from tests.test_gpu_losses import _golden_batch, _model
        g = gold(f'losses_{CASE}')
        cfg = load_cfg('3dmatch')
        cfg.wt_feature_un = 0.05
        model = _model(cfg, g)
        srcs, tgts, extra = _golden_batch(g, CASE)

        def batch():
            b = {'src_xyz': [torch.from_numpy(s).cuda() for s in srcs], 'tgt_xyz': [torch.from_numpy(t).cuda() for t in tgts]}
            b.update(extra)
            return b
        _shared.update(model=model, batch=batch, params=model.trainable_parameters())
    return _shared['model'], _shared['batch'], _shared['params']


def _step(model, batch, params, **kw):
    for p in model.parameters():
        p.grad = None
    b = batch()
    if kw:
        pred = model.forward_grad(b, **kw)
        losses = model.compute_loss_grad(pred, b)
    else:
        pred, losses = model.training_step(b)
    losses['total'].backward()
    return b, pred, losses, [p.grad.clone() for p in params]


def test_training_step_matches_the_inference_arithmetic_and_fills_every_gradient():
    from regtr_amd import context
    model, batch, params = _setup()
    b, pred, losses, grads = _step(model, batch, params)
    layers = model.head_layers()
    assert layers == [5] and len(params) == len(set(map(id, params)))
    # pred: the fp32x3 inference forward, bit for bit
    b2 = batch()
    dev = b2['src_xyz'][0].device
    with torch.no_grad(), context.forward(dev, f16_pair=False, force_x3=True, status=None):
        want = model._forward(b2, dev)
    B = len(want['src_kp'])
    for k in ('src_feat_un', 'tgt_feat_un', 'src_feat', 'tgt_feat', 'src_kp', 'tgt_kp'):
        for x, y in zip(pred[k], want[k]):
            assert torch.equal(x.detach(), y), k
    for k in ('src_kp_warped', 'tgt_kp_warped', 'src_overlap', 'tgt_overlap'):
        for bb in range(B):
            assert sorted(pred[k][bb]) == layers
            for i in layers:
                assert torch.equal(pred[k][bb][i].detach(), want[k][bb][i]), (k, bb, i)
    assert tuple(pred['pose'].shape) == (1, B, 3, 4) and torch.equal(pred['pose'][0], want['pose'][-1])
    # losses: compute_loss on the same pred and batch
    ref = model.compute_loss(pred, b)
    assert list(losses) == list(ref) == model.loss_keys()
    for k in ref:
        got, w = float(losses[k]), float(ref[k])
        print(f'training_step {k}: {got:.7f} vs compute_loss {w:.7f}')
        assert np.isfinite(got) and abs(got - w) <= 1e-6 * abs(w), k
        if k.startswith('overlap'):
            assert torch.equal(losses[k].detach(), ref[k]), 'the overlap terms are bit-equal'
    # gradients: everything above the backbone, nothing below
    for p, gr in zip(params, grads):
        assert torch.isfinite(gr).all() and gr.abs().max() > 0
    assert all(p.grad is None for p in model.kpf_encoder.parameters())
    named = dict(model.named_parameters())
    above = {k for k in named if not k.startswith('kpf_encoder.')}
    assert {id(named[k]) for k in above} == set(map(id, params))
    # a second identical step: the same bits
    _, _, losses2, grads2 = _step(model, batch, params)
    assert torch.equal(losses['total'].detach(), losses2['total'].detach())
    assert all(torch.equal(x, y) for x, y in zip(grads, grads2))
    # backbone_grad: the hand-off to a backbone backward
    b3, pred3, _, grads3 = _step(model, batch, params, backbone_grad=True)
    fu = pred3['_feats_un']
    assert fu.is_leaf and fu.grad is not None and fu.grad.shape == fu.shape and torch.isfinite(fu.grad).all() and fu.grad.abs().max() > 0
    assert all(torch.equal(x, y) for x, y in zip(grads, grads3))
    assert '_feats_un' not in pred


def test_compute_loss_grad_no_host_sync():
    model, batch, params = _setup()
    b = batch()
    pred = model.forward_grad(b)
    model.compute_loss_grad(pred, b)['total'].backward()            # weight preparation (once per weight version)
    pred = model.forward_grad(b)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = model.compute_loss_grad(pred, b)
        losses['total'].backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(losses['total']) and all(torch.isfinite(p.grad).all() for p in params)


def test_ten_sgd_steps_lower_the_total():
    """Ten plain SGD steps (p -= SGD_LR * p.grad) on the one batch.  SGD_LR = 1e-4: with the seeded weights the first step's gradient
    norm is 121 against a parameter norm of 116 and a total of 11.94.  Measured totals over the ten steps: at 1e-4 a monotone descent
    11.94 -> 4.86; at 3e-4 down to 3.63, then up again; at 1e-3 and above the total jumps up and down between steps (7.10, 7.62, 6.62
    ... 2.80).  1e-4 is the largest of the tried step sizes at which every step lowers the total."""
    model, batch, params = _setup()
    state = [p.detach().clone() for p in model.parameters()]
    try:
        hist = []
        for _ in range(10):
            _, _, losses, grads = _step(model, batch, params)
            hist.append(losses['total'].detach())
            with torch.no_grad():
                for p, gr in zip(params, grads):
                    p -= SGD_LR * gr
        _, _, losses, _ = _step(model, batch, params)
        hist.append(losses['total'].detach())
        hist = [float(h) for h in hist]
        print('total per step:', ' '.join(f'{h:.5f}' for h in hist))
        assert all(np.isfinite(hist)) and hist[-1] < hist[0]
    finally:
        with torch.no_grad():
            for p, s in zip(model.parameters(), state):
                p.copy_(s)
