"""CPU: the per-element bounds of tests/test_unet_attention_norm.py hold for numpy emulations of the arithmetic the kernels declare, over the inputs of
every case of that module (the largest GroupNorm tensors excepted).  A bound that the declared arithmetic alone can exceed would fail here, without a GPU."""
import test_unet_attention_norm as m


def test_bounds_hold_for_the_cpu_emulations():
    worst, c_max = m.emulate_all()   # (prints the worst error / bound per input family: -s)
    # the c of the attention bound's c 2^-11 A depends on the bound and the inputs alone: above ~4 the check would have no teeth
    assert c_max <= 4.1, c_max
    # attention: the emulation leaves at least a third of the bound unused; normalisations: the half-ulp term of the last rounding is sharp, so their ratios reach 1
    assert all(r <= 0.67 for n, (r, _) in worst.items() if n.startswith("A")), worst
    assert {n[:1] for n in worst} == {"A", "B", "C"}
