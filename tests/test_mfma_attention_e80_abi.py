"""d_head 80 (OPT-2.7B's heads) on the matrix-core attention and the fused PQ loss at M = 10:
what the library accepts, checked without a GPU."""
import pytest


@pytest.fixture(scope='module')
def lib():
    from naive_gpt import ext
    return ext.load_library()


@pytest.mark.parametrize('S,Z', [(512, 64), (80, 8), (2048, 256)])
def test_d_head_80_is_supported(lib, S, Z):
    assert lib.spt_attention_mfma_supported(S, 80, S * Z) == 1


@pytest.mark.parametrize('S,E,Z', [(512, 32, 64), (512, 96, 64), (4096, 80, 64), (4096, 64, 64)])
def test_other_head_sizes_and_long_rows_stay_refused(lib, S, E, Z):
    assert lib.spt_attention_mfma_supported(S, E, S * Z) == 0


def test_pq_loss_takes_ten_subspaces(lib):
    assert lib.spt_pq_loss_workspace_bytes(4096, 10, 16, 8) > 0
    assert lib.spt_pq_loss_workspace_bytes(4096, 10, 16, 16) == 0      # D = 16 stays refused
