"""The CPU side of the stream-order tests (tests/test_gpu_stream_order.py), without a GPU: the chains together declare every
device entry of the header, and the expected values of every chain differ between its two input sets in every compared
array, so that a stale result cannot pass for a fresh one."""
import pytest

import stream_cases as sc_cases


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    return sc_cases.Twins(tmp_path_factory.mktemp("stream_cases"))


def test_every_device_entry_is_in_a_chain():
    """A device entry added to the header without a chain fails here."""
    want, have = sc_cases.device_entries(), sc_cases.declared_symbols()
    assert have == want, f"without a chain: {sorted(want - have)}; not in the header: {sorted(have - want)}"


def test_exclusions_are_declared_and_host_forms_have_device_forms():
    import sea_current_amd as sc
    names = set(sc.EXPORTS)
    assert sc_cases.EXCLUDED <= names
    assert not any(n.endswith("_host") for n in sc_cases.device_entries())


@pytest.mark.parametrize("chain", sc_cases.CHAINS, ids=lambda c: c.name)
def test_expected_values_differ_between_the_input_sets(twins, chain):
    form = lambda which: {k: (v.shape, v.dtype) for k, v in chain.inputs(which).items()}
    assert form("A") == form("B") == form("C")              # one set overwrites the other in place
    assert set(chain.symbols) <= sc_cases.device_entries()
    chain.differs(twins)
