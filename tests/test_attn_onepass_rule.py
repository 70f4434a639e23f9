"""CPU: ops.attn_bwd_onepass_fits, the Python mirror of the rule in csrc/attention.hip (onepass_fits) that sends a backward
attention to the one-pass kernel: a function of the padded row counts and the head widths against the 80 KB LDS budget."""
import pytest

from deepavfusion_amd import ops


@pytest.mark.parametrize('Nq,Nk,dqk,dv,lds,fits', [
    (63, 95, 64, 64, 41472, True),        # audio tower, ViT-B / ViT-L
    (49, 81, 64, 64, 41472, True),        # image tower
    (80, 112, 64, 64, 66304, True),       # base_m75: 80 audio tokens
    (8, 63, 64, 64, 20736, True),         # aggregations
    (8, 49, 64, 64, 20736, True),
    (16, 64, 16, 64, 14592, True),        # pair attention
    (1, 1, 64, 64, 14592, True),
    (96, 128, 64, 64, 66304, True),       # the largest padded 64-wide problem with Nk <= 128
    (97, 128, 64, 64, 82944, False),      # pads to 128 x 128: 1 KB over
    (64, 160, 64, 64, 57856, True),
    (64, 288, 64, 64, 90624, False),
    (352, 352, 64, 64, 385792, False),    # evaluation-length audio
])
def test_lds_and_rule(Nq, Nk, dqk, dv, lds, fits):
    assert ops.attn_bwd_onepass_lds(Nq, Nk, dqk, dv) == lds
    assert ops.attn_bwd_onepass_fits(Nq, Nk, dqk, dv) is fits


@pytest.mark.parametrize('Nq,Nk,dqk,dv', [(228, 228, 32, 32), (352, 352, 32, 32), (49, 49, 32, 32), (32, 112, 16, 16), (8, 8, 16, 16)])
def test_other_head_widths_keep_the_kernel_pair(Nq, Nk, dqk, dv):
    assert not ops.attn_bwd_onepass_fits(Nq, Nk, dqk, dv)


def test_rule_is_monotone_in_the_row_counts():
    for dqk in (16, 64):
        for nq in range(1, 200, 7):
            prev = True
            for nk in range(1, 400, 13):
                now = ops.attn_bwd_onepass_fits(nq, nk, dqk, 64)
                assert prev or not now, (nq, nk, dqk)
                prev = now
