"""Host-side checks of the loss entry points (no GPU needed): argument refusals that launch nothing, the loss weights and the restated
`losses:` config values against the reference's numbers, and test.py's --losses refusal for ModelNet."""
import os
import subprocess
import sys

import pytest

from tests.util import ROOT, load_cfg


def _lib():
    from regtr_amd import _lib as L
    return L.lib()


FAKE = 0x10000          # never dereferenced: every call below is refused before a launch


def _infonce(D=256, n_pairs=1, n_anc=4, n_pos=4, max_anc=4, anc=FAKE, pos=FAKE, axyz=FAKE, pxyz=FAKE, aoff=FAKE, poff=FAKE, out=FAKE,
             ws=FAKE, lda=None, ldp=None, ws_bytes=1 << 20):
    return _lib().regtr_infonce(anc, lda or D, pos, ldp or D, axyz, pxyz, aoff, poff, n_pairs, n_anc, n_pos, max_anc, D, 0.2, 0.4,
                                None, out, None, None, ws, ws_bytes, None)


@pytest.mark.parametrize('D', [0, 32, 100, 576, 1024, -64])
def test_infonce_refuses_bad_D(D):
    assert _infonce(D=D) == -2


@pytest.mark.parametrize('kw', [{'n_pairs': -1}, {'n_anc': -1}, {'n_pos': -3}, {'max_anc': -1}])
def test_infonce_refuses_negative_counts(kw):
    assert _infonce(**kw) == -2


@pytest.mark.parametrize('kw', [{'anc': None}, {'pos': None}, {'axyz': None}, {'pxyz': None}, {'aoff': None}, {'poff': None},
                                {'out': None}, {'ws': None}])
def test_infonce_refuses_null_with_count(kw):
    assert _infonce(**kw) == -2


def test_infonce_refuses_bad_strides_and_alignment():
    assert _infonce(lda=255) == -2                           # ld < D
    assert _infonce(lda=258) == -2                           # rows not 16-byte aligned
    assert _infonce(anc=FAKE + 4) == -2
    assert _infonce(ws_bytes=0) == -3                        # workspace too small


def test_infonce_nothing_to_do_is_ok():
    assert _infonce(n_pairs=0, n_anc=0, n_pos=0, max_anc=0, anc=None, pos=None, axyz=None, pxyz=None, aoff=None, poff=None,
                    out=None, ws=None) == 0
    assert _lib().regtr_infonce_ws_bytes(3, 100) == 3 * 4 * 16
    assert _lib().regtr_infonce_ws_bytes(-1, 100) == 0


def test_loss_terms_refusals():
    L = _lib()
    f = lambda **k: L.regtr_loss_terms(k.get('logit', FAKE), k.get('gt', FAKE), k.get('kp', FAKE), k.get('warped', FAKE),
                                       k.get('seg', FAKE), k.get('B', 1), k.get('N', 8), k.get('pose', FAKE), k.get('ps', 12),
                                       k.get('out', FAKE), None)
    assert f(B=-1) == -2 and f(N=-1) == -2
    assert f(ps=9) == -2
    for k in ('logit', 'gt', 'kp', 'warped', 'seg', 'pose', 'out'):
        assert f(**{k: None}) == -2, k
    assert f(B=0, N=0, logit=None, gt=None, kp=None, warped=None, seg=None, pose=None, out=None) == 0
    assert L.regtr_se3_transform(FAKE, FAKE, 1, -1, FAKE, 12, FAKE, None) == -2
    assert L.regtr_se3_transform(FAKE, FAKE, 1, 4, FAKE, 13, FAKE, None) == -2
    assert L.regtr_se3_transform(None, FAKE, 1, 4, FAKE, 12, FAKE, None) == -2


# reference src/conf/*.yaml `losses:` sections and regtr.py:90-95, restated
REF_LOSSES = {
    '3dmatch': dict(wt_overlap=1.0, overlap_loss_pyr=3, overlap_loss_on=[5], wt_feature=0.1, wt_feature_un=0.0, r_p=0.2, r_n=0.4,
                    feature_loss_on=[5], feature_loss_type='infonce', wt_corr=1.0, corr_loss_on=[5]),
    'modelnet': dict(wt_overlap=1.0, overlap_loss_pyr=3, overlap_loss_on=[5], wt_feature=0.1, wt_feature_un=0.0, r_p=0.12, r_n=0.24,
                     feature_loss_on=[5], feature_loss_type='infonce', wt_corr=1.0, corr_loss_on=[5]),
}


@pytest.mark.parametrize('name', ['3dmatch', 'modelnet'])
def test_loss_config_and_weight_dict(name):
    from regtr_amd.regtr import loss_weight_dict
    cfg = load_cfg(name)
    for k, v in REF_LOSSES[name].items():
        assert cfg[k] == v, k
    wd = loss_weight_dict(cfg)
    assert wd == {'overlap_5': 1.0, 'feature_5': 0.1, 'corr_5': 1.0, 'feature_un': 0.0}
    assert list(wd) == ['overlap_5', 'feature_5', 'corr_5', 'feature_un']
    # keys absent: the reference's default layer list (num_encoder_layers - 1)
    cfg2 = dict(cfg)
    del cfg2['corr_loss_on']
    from regtr_amd.config import as_config
    assert loss_weight_dict(as_config(cfg2))['corr_5'] == 1.0


def test_compute_loss_needs_the_losses_section():
    from regtr_amd import RegTR
    cfg = load_cfg('3dmatch')
    for k in ('r_p', 'r_n'):
        c = dict(cfg)
        del c[k]
        m = RegTR(c)
        with pytest.raises(KeyError, match=k):
            m.compute_loss({'src_kp': []}, {})
    c = dict(cfg)
    c['feature_loss_type'] = 'circle'
    with pytest.raises(NotImplementedError):
        RegTR(c).compute_loss({'src_kp': []}, {})


def test_test_py_refuses_losses_for_modelnet(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'test.py'), '--config', os.path.join(ROOT, 'regtr_amd', 'conf', 'modelnet.yaml'),
           '--benchmark', 'ModelNet', '--synthetic', '2', '--losses', '--logdir', str(tmp_path), '--num_workers', '0']
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert '--losses' in (r.stdout + r.stderr) and 'ModelNet' in (r.stdout + r.stderr)
