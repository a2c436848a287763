"""CloudBank: what `RegTR.encode_clouds` keeps of every cloud, so that `RegTR.register` can pair each cloud any number of times.

Everything RegTR computes before the cross-encoder is a function of ONE cloud: the voxel pyramid, the eleven KPConv blocks (their
InstanceNorm is per cloud), feat_proj and the positional embedding.  A bank holds those results for C clouds, packed back to back on
the device:

    xyz     (N, 3)   the coarsest key points
    feats   (N, D)   feat_proj's output (the dict's '*_feat_un')
    pe      (N, D)   the positional embedding of xyz, or None when the model reads none
    seg_off (C + 1,) int32, device: cloud c owns rows seg_off[c] .. seg_off[c + 1]
    lens             the same lengths on the host (a tuple of ints): no call here waits for the device

and a STAMP of the model it came from: the model's identity and the version counters of every kpf_encoder / feat_proj / pos_embed
parameter.  An optimiser step or a load_state_dict advances those counters, and `check(model)` -- which RegTR.register calls before
its first launch -- then refuses the bank: stale features are an error, never a silent result.

What the stamp cannot see: a write that goes around torch's version counter (`p.data.copy_(...)`, a kernel writing through a raw
pointer without torch.autograd.graph.increment_version), and another model object that Python created at a collected model's address.
Code that edits weights that way must encode again on its own account.

`cat` joins banks, `select` keeps / reorders / repeats clouds (one regtr_gather_segments launch; what an LRU eviction runs).
"""
import torch

from . import context, ops


def model_stamp(model):
    """(id(model), (data_ptr, version counter) of every kpf_encoder / feat_proj / pos_embed parameter): changes whenever a weight the
    bank's contents depend on is written through torch (optimizer.step(), load_state_dict, .to(), an in-place op on the parameter) --
    not by a write through `p.data` or a raw pointer, which advances no counter (the module docstring)."""
    mods = (model.kpf_encoder, model.feat_proj, model.pos_embed)
    return (id(model), tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters()))


def upload_tables(lens, cloud_of, device):
    """The tables of one regtr_gather_segments launch over a bank with host lengths `lens`: -> (dst_seg (n_dst + 1,), cloud_of (n_dst,),
    n_out, max_len), the two int32 device tensors views of ONE buffer that goes up in ONE pinned, non-blocking copy."""
    sel = [int(lens[c]) for c in cloud_of]
    seg = [0]
    for n in sel:
        seg.append(seg[-1] + n)
    host = torch.tensor(seg + [int(c) for c in cloud_of], dtype=torch.int32).pin_memory()
    tab = host.to(device, non_blocking=True)
    return tab[:len(seg)], tab[len(seg):], seg[-1], max(sel, default=0)


class CloudBank:
    __slots__ = ('xyz', 'feats', 'pe', 'seg_off', 'lens', 'stamp')

    def __init__(self, xyz, feats, pe, seg_off, lens, stamp):
        self.xyz, self.feats, self.pe, self.seg_off = xyz, feats, pe, seg_off
        self.lens = tuple(int(n) for n in lens)
        self.stamp = stamp

    def __len__(self):
        return len(self.lens)

    @property
    def device(self):
        return self.feats.device

    @property
    def nbytes(self):
        """Device bytes the bank's rows and offsets occupy."""
        return sum(t.numel() * t.element_size() for t in (self.xyz, self.feats, self.pe, self.seg_off) if t is not None)

    def check(self, model, what='CloudBank'):
        """Raises unless this bank was encoded by `model` with the weights it holds now, on the device it lives on."""
        if self.stamp[0] != id(model):
            raise RuntimeError(f'{what}: the bank was encoded by another model')
        if self.device != model.device:
            raise RuntimeError(f'{what}: the bank lives on {self.device}, the model on {model.device}')
        if self.stamp != model_stamp(model):
            raise RuntimeError(f'{what}: the bank is stale -- a kpf_encoder / feat_proj / pos_embed weight changed since encode_clouds '
                               '(optimizer.step(), load_state_dict, .to()); encode the clouds again')

    @staticmethod
    def cat(banks):
        """The clouds of `banks`, in order, as one bank.  All must come from one model state and one device."""
        banks = list(banks)
        if not banks:
            raise ValueError('CloudBank.cat: no banks')
        b0 = banks[0]
        for b in banks[1:]:
            if b.stamp != b0.stamp:
                raise RuntimeError('CloudBank.cat: the banks come from different models or from different weights of one model')
            if b.device != b0.device or (b.pe is None) != (b0.pe is None):
                raise RuntimeError('CloudBank.cat: the banks live on different devices or only some carry a positional embedding')
        if len(banks) == 1:
            return b0
        lens = tuple(n for b in banks for n in b.lens)
        # the offsets from the banks' own device tables (a running base each, known to the host): no upload, no wait
        base, segs = 0, [b0.seg_off[:1]]
        for b in banks:
            segs.append(b.seg_off[1:] + base if base else b.seg_off[1:])
            base += sum(b.lens)
        return CloudBank(torch.cat([b.xyz for b in banks]), torch.cat([b.feats for b in banks]),
                         None if b0.pe is None else torch.cat([b.pe for b in banks]), torch.cat(segs), lens, b0.stamp)

    def select(self, indices):
        """The clouds `indices` (host ints; any order, repeats allowed) as a new bank: one upload of the tables, one
        regtr_gather_segments launch.  Dropping clouds = selecting the ones to keep."""
        idx = [int(i) for i in indices]
        bad = [i for i in idx if not 0 <= i < len(self)]
        if bad:
            raise IndexError(f'CloudBank.select: cloud {bad[0]} is not in a bank of {len(self)}')
        dev = self.device
        with context.on_device(dev):
            seg, cloud_of, n_out, max_len = upload_tables(self.lens, idx, dev)
            feats, pe, xyz = ops.gather_segments(self.feats, self.seg_off, cloud_of, seg, n_out, max_len, pe=self.pe, xyz=self.xyz)
        return CloudBank(xyz, feats, pe, seg, [self.lens[i] for i in idx], self.stamp)
