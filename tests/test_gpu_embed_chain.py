"""The fixed-order embedding gradient on the GPU, bit for bit against the NumPy float32 replay of its association
(tests/embed_chain_cases.py); emulator twin: tests/test_embed_chain_emu.py."""
import pytest

from tests.embed_chain_cases import CASES, DIMS, chain_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("sets", [pytest.param(s, id=i) for i, s in CASES])
def test_embed_chain_replay(hip, sets, d):
    chain_case(hip, d, sets)
