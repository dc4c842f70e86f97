"""Evaluation metrics without any back end: the product path refuses CPU tensors, and the SSIM window is the documented one."""
import math

import pytest
import torch


def test_product_path_has_no_cpu_fallback():
    from bbdm_amd import _lib, metrics
    a = torch.zeros(1, 11, 11, 3, dtype=torch.uint8)
    with pytest.raises(_lib.BBDMHipError):
        metrics.pair_metrics(a, a)
    with pytest.raises(_lib.BBDMHipError):
        metrics.diversity(a.unsqueeze(0))
    with pytest.raises(_lib.BBDMHipError):
        metrics.SetEvaluator(2).add_sample(0, 0, torch.zeros(3, 11, 11))


def test_ssim_window_is_the_normalised_gaussian():
    from bbdm_amd import metrics
    w = metrics.ssim_window()
    assert len(w) == 11 and all(w[i] == w[10 - i] for i in range(11)) and abs(math.fsum(w) - 1.0) <= 2 ** -52
    assert w[5] / w[4] == pytest.approx(math.exp(1.0 / 4.5), rel=1e-15)


def test_public_names_are_exported():
    import bbdm_amd
    for name in ("pair_metrics", "diversity", "SetEvaluator", "metrics_from_dirs"):
        assert getattr(bbdm_amd, name) is getattr(bbdm_amd.metrics, name) and name in bbdm_amd.__all__
