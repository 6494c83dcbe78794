"""Host side of the position-table gradients for any relative-position map (no GPU): the delta lists fbl_attn_pos_grad
reads cover every relative position exactly once, and only the default call keeps the walking kernel's limit."""
import types

import numpy as np
import pytest
import torch

from frozenbilm_amd.attn_bwd import POS_GRAD_MAX_DELTAS, _delta_ranges, _relidx_range
from frozenbilm_amd.model.relpos import rel_index_vector

MAPS = [(64, 512, 266), (64, 512, 512), (128, 512, 512), (32, 128, 128), (0, 128, 300), (0, 128, 512), (256, 512, 512)]


def _map(pb, mr):
    return types.SimpleNamespace(position_buckets=pb, max_rel=mr, att_span=pb if pb > 0 else mr)


@pytest.mark.parametrize("pb,mr,S", MAPS)
def test_delta_ranges_without_limit_cover_every_delta_once(pb, mr, S):
    cfg = _map(pb, mr)
    cpu = torch.device("cpu")
    dlo, dcnt, cmax = _delta_ranges(S, cfg, cpu, limit=None)
    rmin, rcnt = _relidx_range(S, cfg)
    rv = rel_index_vector(S, pb, mr, cfg.att_span).astype(np.int64)
    assert dlo.dtype == dcnt.dtype == torch.int16 and dlo.numel() == dcnt.numel() == rcnt
    assert cmax == int(dcnt.max())
    seen = np.zeros(2 * S - 1, dtype=np.int64)
    for r in range(rcnt):
        for d in range(int(dlo[r]), int(dlo[r]) + int(dcnt[r])):
            assert rv[d + S - 1] == rmin + r, (r, d)
            seen[d + S - 1] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("pb,mr,S,peak", [(64, 512, 266, 21), (64, 512, 512, 44), (128, 512, 512, 17), (32, 128, 128, 17),
                                          (0, 128, 300, 173), (0, 128, 512, 385)])
def test_default_call_keeps_the_walking_kernel_limit(pb, mr, S, peak):
    """the largest delta count of each map (the table of the issue), and the default call still refusing it -- also after a
    call without a limit has cached the lists"""
    cfg = _map(pb, mr)
    cpu = torch.device("cpu")
    assert _delta_ranges(S, cfg, cpu, limit=None)[2] == peak > POS_GRAD_MAX_DELTAS
    with pytest.raises(NotImplementedError, match=rf"at most {POS_GRAD_MAX_DELTAS} .* puts {peak} on one row"):
        _delta_ranges(S, cfg, cpu)
    assert _delta_ranges(S, cfg, cpu, limit=peak)[2] == peak
