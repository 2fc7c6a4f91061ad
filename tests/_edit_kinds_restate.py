"""A plain-torch restatement of the edit operator (``dmnerf_edit_exchange``: the three kinds plus the keep mask) and the seeded
fixture its tests share.  tests/test_edit_kinds_restate.py pins the restatement to ``oracle.ref_cpu.exchanger`` -- itself pinned
to the reference -- and tests/test_gpu_edit_kinds.py holds the kernel to the restatement bit for bit.

The label decisions are ``torch.argmax(torch.sigmoid(.))`` as the reference writes them; their tie rule (the first maximum) is
the CPU's, so the restatement is always evaluated on host tensors."""
import torch

MOVE, COPY, REMOVE = 0, 1, 2
BRANCHES = ("occlusion", "fill", "exchange1", "exchange3", "eliminate", "copy", "copy_skip", "remove", "keep_zero")


def edit_restate(ori_raw, tar_raws, ori_acc, tar_accs, labels, kinds, keep_labels=None, counts=None):
    """``ori_raw [N,S,4+C]`` is edited in place -> ``(ori_raw, ori_label [N,S])``.  ``counts`` (a dict): how many rows took each
    branch of ``BRANCHES`` is added to it."""
    assert ori_raw.device.type == "cpu"
    count = (lambda k, m: counts.__setitem__(k, counts.get(k, 0) + int(m.sum()))) if counts is not None else (lambda k, m: None)
    S, C = ori_raw.shape[1], ori_raw.shape[2] - 4
    l0 = torch.argmax(torch.sigmoid(ori_raw[..., 4:]), dim=-1)
    ori_lab = l0.clone()
    if len(labels):
        acc_lab = torch.argmax(torch.sigmoid(ori_acc[..., :-1]), dim=-1)[:, None].repeat(1, S)
    for e, (L, kind) in enumerate(zip(labels, kinds)):
        occluded = (acc_lab != L) & (ori_lab == L)
        ori_lab[occluded] = acc_lab[occluded]
        count("occlusion", occluded)
        ori_is = ori_lab == L
        if kind == REMOVE:
            ori_raw[ori_is] = ori_raw[ori_is] * 0
            count("remove", ori_is)
            continue
        assert kind in (MOVE, COPY)
        tar_raw = tar_raws[e]
        tar_lab = torch.argmax(torch.sigmoid(tar_raw[..., 4:]), dim=-1)
        tar_acc_lab = torch.argmax(torch.sigmoid(tar_accs[e][..., :-1]), dim=-1)[:, None].repeat(1, S)
        tar_occluded = (tar_acc_lab != L) & (tar_lab == L)
        tar_lab[tar_occluded] = tar_acc_lab[tar_occluded]
        tar_is = tar_lab == L
        if kind == MOVE:
            fill = (acc_lab == L) & ~ori_is
            take = fill | tar_is                         # fill, reduced == 1, reduced == 3
            eliminate = ori_is & ~tar_is                 # reduced == 2
            ori_raw[take] = tar_raw[take]
            ori_raw[eliminate] = ori_raw[eliminate] * 0
            count("fill", fill); count("exchange1", tar_is & ~ori_is); count("exchange3", tar_is & ori_is); count("eliminate", eliminate)
        else:
            take = tar_is & ~ori_is                      # reduced == 1 only
            ori_raw[take] = tar_raw[take]
            count("copy", take); count("copy_skip", tar_is & ori_is)
    if keep_labels is not None:
        keep = torch.zeros(C, dtype=torch.bool)
        keep[[int(l) for l in keep_labels]] = True
        drop = ~keep[l0]
        ori_raw[drop] = ori_raw[drop] * 0
        count("keep_zero", drop)
    return ori_raw, ori_lab


def _rows(g, lead, lab, C):
    """Logits ``[*lead, C]`` whose largest is at ``lab`` (6 .. 7 there, standard normal elsewhere)."""
    x = torch.randn(*lead, C, generator=g)
    x.scatter_(-1, lab[..., None], 6.0 + torch.rand(*lead, 1, generator=g))
    return x


def _pick(g, lead, hi, labels, ray=None):
    """Labels in ``[0, hi)``, so mixed that every branch has rows: a third the ray's own label (``ray [N]``, if given), a third
    drawn from the edited ``labels``, the rest uniform."""
    u = torch.randint(0, hi, lead, generator=g)
    r = torch.rand(*lead, generator=g)
    if len(labels):
        own = torch.tensor(labels)[torch.randint(0, len(labels), lead, generator=g)].clamp(max=hi - 1)
        u = torch.where(r < 0.7, own, u)
    if ray is not None:
        u = torch.where(r < 0.35, ray.clamp(max=hi - 1).reshape(-1, *[1] * (len(lead) - 1)).expand(*lead), u)
    return u


def _acc(g, lab, C):
    """An accumulated map ``[N, C]`` of ray labels ``lab`` (< C - 1); on every other ray the LAST channel is the largest of all,
    which the operator must not see (it takes the argmax over C - 1 channels)."""
    x = _rows(g, tuple(lab.shape), lab, C)
    x[::2, -1] = 9.0
    return x


def _ray_labels(g, N, C, labels):
    """Ray labels: rays 1, 2, ... carry the edited labels in turn (a short batch still has a ray of the first edits)."""
    la = _pick(g, (N,), C - 1, labels)
    for i, L in enumerate(labels[:max(N - 2, 0)]):
        la[1 + i] = min(L, C - 2)
    return la


def make_case(N, S, C, labels, kinds, seed, inf_label=None):
    """A seeded case with planted rows -> dict(ori, tars, ori_acc, tar_accs); targets are ``None`` for a REMOVE.

    Planted in ray 0 (S >= 2): sample 0 has an exact logit tie between channels 0 and C - 1; sample 1 has logits 21 at channel 0 and
    30 at channel C - 1, both sigmoids are 1.0f, so the label is 0 (first maximum) although the larger logit is the last.  Ray 0's
    accumulated label is 0.  ``inf_label``: the last sample of the last ray carries that label (so does its ray) and an ``inf``
    colour: once zeroed it holds NaN."""
    g = torch.Generator().manual_seed(seed)
    la = _ray_labels(g, N, C, labels)
    ori = torch.cat([torch.randn(N, S, 4, generator=g), _rows(g, (N, S), _pick(g, (N, S), C, labels, la), C)], -1)
    ori_acc = _acc(g, la, C)
    tars, tar_accs = [], []
    for kind in kinds:
        if kind == REMOVE:
            tars.append(None); tar_accs.append(None)
            continue
        lta = torch.where(torch.rand(N, generator=g) < 0.6, la, _pick(g, (N,), C - 1, labels))      # often the original ray's label
        tars.append(torch.cat([torch.randn(N, S, 4, generator=g), _rows(g, (N, S), _pick(g, (N, S), C, labels, lta), C)], -1))
        tar_accs.append(_acc(g, lta, C))
    if S >= 2:
        ori[0, 0, 4:] = torch.randn(C, generator=g).clamp(max=3.0)
        ori[0, 0, 4] = ori[0, 0, 4 + C - 1] = 8.0
        ori[0, 1, 4:] = torch.randn(C, generator=g).clamp(max=3.0)
        ori[0, 1, 4], ori[0, 1, 4 + C - 1] = 21.0, 30.0
        ori_acc[0, :C - 1] = torch.randn(C - 1, generator=g).clamp(max=3.0)
        ori_acc[0, 0] = 7.5
    if inf_label is not None:
        ori[N - 1, S - 1, 4:] = 0.0
        ori[N - 1, S - 1, 4 + inf_label] = 9.0
        ori_acc[N - 1, :C - 1] = 0.0
        ori_acc[N - 1, inf_label] = 9.0
        ori[N - 1, S - 1, 1] = float("inf")
    return dict(ori=ori, tars=tars, ori_acc=ori_acc, tar_accs=tar_accs)


def bits(t):
    return t.contiguous().view(torch.int32)
