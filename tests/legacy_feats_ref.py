"""Plain-torch fp64 restatement of the six-map norm_add (the `feats` of the legacy head layout): the rounding-free model of tests/test_legacy_feats_gpu.py."""
import torch.nn.functional as F


def norm_add6_ref(maps):
    """maps: NCHW tensors, the first one at the output size -> the mean of the L2-normalised (over channels), bilinearly resized maps, fp64"""
    xs = [F.normalize(x.double(), p=2, dim=1) for x in maps]
    xs = [F.interpolate(x, size=xs[0].shape[-2:], mode='bilinear', align_corners=False) for x in xs]
    return sum(xs) / len(xs)
