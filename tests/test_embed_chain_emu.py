"""The fixed-order embedding gradient on the host emulation, bit for bit against the NumPy float32 replay of its association
(tests/embed_chain_cases.py); GPU twin: tests/test_gpu_embed_chain.py."""
import pytest

from tests.embed_chain_cases import CASES, DIMS, chain_case


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("sets", [pytest.param(s, id=i) for i, s in CASES])
def test_embed_chain_replay(emu, sets, d):
    chain_case(emu, d, sets)
