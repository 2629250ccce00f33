"""The two-plane fp16 format's scale rule at its boundaries without a GPU: the CPU build's mms_split_planes16_group gives exactly
2^(14 - e) per row and the planes of a numpy float16 emulation of the hi / lo rule, bit for bit (tests/planes16_check.py)."""
import pytest

import planes16_check as pc


@pytest.mark.parametrize("K", pc.WIDTHS)
def test_cpu_build_scales_and_planes_at_the_boundaries(K):
    pc.check_cpu_build(K)
