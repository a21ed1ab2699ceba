"""CPU-only: the cache-policy mask of the C ABI (pk_set_cache_policy / pk_get_cache_policy) -- layout of the Python helper, round trip,
refusal of masks that name no site or policy.  No kernel is launched."""
import pytest


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    return _lib


def test_mask_helper_layout(L):
    assert L.CP_SITES == ('gemm', 'qkv_attn', 'peg', 'ln', 'patch_wide', 'patch_finish', 'ld_video', 'ld_partials', 'ld_residual')
    assert L.cache_policy_mask() == 0
    assert L.cache_policy_mask(gemm=L.CP_WT) == 1 and L.cache_policy_mask(peg=L.CP_NT) == 2 << 4
    assert L.cache_policy_mask(ld_residual=L.CP_NT, qkv_attn=L.CP_WT) == (2 << 16) | (1 << 2)
    with pytest.raises(ValueError):
        L.cache_policy_mask(nowhere=1)


def test_set_get_round_trip_and_refusals(L):
    saved = L.get_cache_policy()
    try:
        for mask in (0, L.cache_policy_mask(peg=L.CP_WT, ln=L.CP_NT, ld_video=L.CP_NT), 0b10_10_10_01_01_01_01_01_01, 0b10_10_10_10_10_10_10_10_10):
            L.set_cache_policy(mask)
            assert L.get_cache_policy() == mask
        for bad in (3, 3 << 6, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 31):      # policy 3, write-through loads, bits past the last site
            with pytest.raises(RuntimeError, match='PK_EINVAL'):
                L.set_cache_policy(bad)
            assert L.get_cache_policy() == 0b10_10_10_10_10_10_10_10_10
    finally:
        L.set_cache_policy(saved)
