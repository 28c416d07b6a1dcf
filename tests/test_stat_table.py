"""_lib.STATS, the one table of the five draw statistics: the names derived from it are the names include/hmcg.h declares, and
every make_* fills its struct as a struct filled by hand.  No GPU, no library call."""
import ctypes as C

import pytest

from hmc_jl_amd import _lib


def test_exports_are_what_they_were():
    assert _lib.EXPORTS == (
        "hmcg_version", "hmcg_device_count", "hmcg_last_error", "hmcg_shutdown",
        "hmcg_estimate_batch", "hmcg_estimate_batch_device", "hmcg_estimate_batch_multi",
        "hmcg_save_results_csv", "hmcg_write_table_csv", "hmcg_format_float",
        "hmcg_predictive_cdf", "hmcg_predictive_cdf_device", "hmcg_bias_moments", "hmcg_bias_moments_device",
        "hmcg_mixture_moments", "hmcg_mixture_moments_device", "hmcg_chain_density", "hmcg_chain_density_device",
        "hmcg_chain_autocorr", "hmcg_chain_autocorr_device")


def _by_hand(cls, **fields):
    p = cls()
    p.struct_size = C.sizeof(cls)
    for name, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(p, name)[i] = x
        else:
            setattr(p, name, v)
    return p


CASES = [
    (lambda: _lib.make_predictive(5, 3, 1000, 1024, 81, (0, 12), device=2),
     lambda: _by_hand(_lib.Predictive, W=5, K=3, device=2, nd=1000, nd_ld=1024, G=81, n_h=2, horizons=(0, 12), flags=1)),
    (lambda: _lib.make_bias(5, 4, 1000, 1024, 12, 2, device=1, round5=False),
     lambda: _by_hand(_lib.Bias, W=5, K=4, device=1, nd=1000, nd_ld=1024, horizon=12, H=2, flags=0)),
    (lambda: _lib.make_mixmom(7, 2, 300, 300, (12, 0, 3), device=3),
     lambda: _by_hand(_lib.MixMom, W=7, K=2, device=3, nd=300, nd_ld=300, n_h=3, horizons=(12, 0, 3), flags=1)),
    (lambda: _lib.make_density(2, 9, 5000, 6000, (1000, 5000), 32, (10, 100), device=1),
     lambda: _by_hand(_lib.Density, W=2, C=9, device=1, nd=5000, nd_ld=6000, B=32, n_cuts=2, cuts=(1000, 5000), trace_len=10,
                      trace_stride=100, flags=1)),
    (lambda: _lib.make_density(2, 9, 5000, 6000, round5=False),
     lambda: _by_hand(_lib.Density, W=2, C=9, nd=5000, nd_ld=6000, B=64, n_cuts=1, cuts=(5000,), trace_len=0, trace_stride=1)),
    (lambda: _lib.make_autocorr(3, 16, 4000, 4096, 100, device=2),
     lambda: _by_hand(_lib.Autocorr, W=3, C=16, device=2, nd=4000, nd_ld=4096, L=100, flags=1)),
]


@pytest.mark.parametrize("made, by_hand", CASES)
def test_make_fills_the_struct_as_by_hand(made, by_hand):
    got, want = made(), by_hand()
    assert type(got) is type(want)
    for name, ctype in got._fields_:
        a, b = getattr(got, name), getattr(want, name)
        if issubclass(ctype, C.Array):
            a, b = list(a), list(b)
        assert a == b, name
    assert bytes(got) == bytes(want)                           # ... and nothing between the fields


def test_the_table_names_the_five_structs_and_flags():
    assert [(s.struct, s.stem, s.round5) for s in _lib.STATS.values()] == [
        (_lib.Predictive, "predictive_cdf", 1), (_lib.Bias, "bias_moments", 1), (_lib.MixMom, "mixture_moments", 1),
        (_lib.Density, "chain_density", 1), (_lib.Autocorr, "chain_autocorr", 1)]
    with pytest.raises(ValueError, match="at most 8 horizons"):
        _lib.make_predictive(1, 3, 4, 4, 2, tuple(range(9)))
    with pytest.raises(ValueError, match="at most 8 horizons"):
        _lib.make_mixmom(1, 3, 4, 4, tuple(range(9)))
