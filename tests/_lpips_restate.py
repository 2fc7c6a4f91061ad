"""Plain-torch restatement of the LPIPS definition the package implements (lpips 0.1.4, ``net='vgg'``, ``version='0.1'``,
``spatial=False``; written down without the library at hand, as csrc/lpips.hip's header says), parametrised by dtype: the float64
run is the referee of tests/test_gpu_lpips.py, the float32 run the measure of what float32 arithmetic can deliver.  Also the
random-weight generator all LPIPS tests share.  Nothing here constructs ``lpips.LPIPS`` or a torchvision model."""
import math

import torch
import torch.nn.functional as F

# (index in vgg16().features, slice, Cin, Cout)
CONVS = ((0, 1, 3, 64), (2, 1, 64, 64), (5, 2, 64, 128), (7, 2, 128, 128), (10, 3, 128, 256), (12, 3, 256, 256), (14, 3, 256, 256),
         (17, 4, 256, 512), (19, 4, 512, 512), (21, 4, 512, 512), (24, 5, 512, 512), (26, 5, 512, 512), (28, 5, 512, 512))
TAPS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def random_state_dict(seed=0, bias_std=0.05):
    """A state dict in ``lpips.LPIPS(net='vgg').state_dict()``'s form with random float32 weights: He-normal convolutions (std =
    sqrt(2 / (9 Cin)), so the activations neither die nor blow up over 13 layers), small biases, non-negative ``lin`` weights."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, sl, cin, cout in CONVS:
        sd[f"net.slice{sl}.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"net.slice{sl}.{idx}.bias"] = torch.randn(cout, generator=g) * bias_std
    for k, c in enumerate(TAPS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g)
    return sd


def maxpool_floor(x):
    """2x2 / stride 2 maximum of ``[N,C,H,W]``; an odd last row or column is dropped."""
    return F.max_pool2d(x, kernel_size=2, stride=2)


def features(x, sd, dtype):
    """The five tapped feature maps ``[N,C,h,w]`` of frames ``x [N,H,W,3]`` (as given: no 2x-1)."""
    x = x.to(dtype).permute(0, 3, 1, 2)
    x = (x - torch.tensor(SHIFT, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dtype).view(1, 3, 1, 1)
    taps = []
    for i, (idx, sl, cin, cout) in enumerate(CONVS):
        if i > 0 and CONVS[i - 1][1] != sl:
            x = maxpool_floor(x)
        x = F.relu(F.conv2d(x, sd[f"net.slice{sl}.{idx}.weight"].to(dtype), sd[f"net.slice{sl}.{idx}.bias"].to(dtype), padding=1))
        if i + 1 == len(CONVS) or CONVS[i + 1][1] != sl:
            taps.append(x)
    return taps


def lpips_restate(pred, gt, sd, dtype=torch.float64, normalize=False):
    """``(feats, score)``: ``feats`` five maps ``[2P,h,w,C]`` (pred frames, then gt frames), ``score [P]``, all in ``dtype``."""
    single = pred.dim() == 3
    if single:
        pred, gt = pred[None], gt[None]
    P = pred.shape[0]
    x = torch.cat([pred, gt], 0).to(dtype)
    if normalize:
        x = 2 * x - 1
    taps = features(x, sd, dtype)
    score = torch.zeros(P, dtype=dtype)
    for k, f in enumerate(taps):
        f0, f1 = f[:P], f[P:]
        n0 = torch.sqrt((f0 ** 2).sum(1, keepdim=True))
        n1 = torch.sqrt((f1 ** 2).sum(1, keepdim=True))
        d = (f0 / (n0 + 1e-10) - f1 / (n1 + 1e-10)) ** 2
        w = sd[f"lin{k}.model.1.weight"].to(dtype)
        score = score + (d * w).sum(1).mean((1, 2))
    feats = [f.permute(0, 2, 3, 1).contiguous() for f in taps]
    return feats, (score[0] if single else score)


def frames(P, H, W, seed):
    """``(pred, gt) [P,H,W,3]`` float32 in [0,1]: gt smooth plus noise, pred = gt + a perturbation."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(3.0 * xx + 2.0 * yy + c) * torch.cos(2.0 * yy - xx + 0.5 * c) for c in range(3)], -1)
    gt = (base[None] + 0.05 * torch.randn(P, H, W, 3, generator=g)).clamp(0, 1)
    pred = (gt + 0.08 * torch.randn(P, H, W, 3, generator=g)).clamp(0, 1)
    return pred.float().contiguous(), gt.float().contiguous()


# The cases of the whole-metric test: (P, H, W, seed).  16 x 16: the last tap is 1 x 1; 37 x 50: odd at every pooling level
# (37 -> 18 -> 9 -> 4 -> 2, 50 -> 25 -> 12 -> 6 -> 3); 96 x 128: many tiles.
METRIC_CASES = ((2, 16, 16, 11), (2, 37, 50, 12), (1, 96, 128, 13))


def rel_feature_error(got, want):
    """max |got - want| over max |want|: the feature maps' measure."""
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())
