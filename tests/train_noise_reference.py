"""NumPy restatement of the per-sample training noise (diffusion_amd/train_noise.py, da_add_noise_rng): the seed derivation,
the timestep formulas and the noise composition, in np.float32 with one rounding per operation.  The Philox stream itself is
tests/philox_reference.py."""
import numpy as np

import philox_reference as PR

SEED_DOMAIN = 0x7472616e
MASK = 0xFFFFFFFF


def sample_seeds(run_seed, batch_idx, first_position, n):
    """seed of global position g: r0 | r1 << 32 of Philox(counter (g, batch lo, batch hi, 'tran'), key = the run's seed)"""
    key = (run_seed & MASK, run_seed >> 32)
    out = []
    for g in range(first_position, first_position + n):
        r = PR.philox4x32_10((g, batch_idx & MASK, batch_idx >> 32, SEED_DOMAIN), key)
        out.append(int(r[0]) | int(r[1]) << 32)
    return out


def timestep_word(seed):
    """r0 of draw 3: counter (0, 3, 0, 0) under the sample's key"""
    return int(PR.philox4x32_10((0, 3, 0, 0), (seed & MASK, seed >> 32))[0])


def discrete_t(r0, t_lo, t_hi, slot=None, n_slots=0):
    R = t_hi - t_lo
    if slot is None:
        return t_lo + ((r0 * R) >> 32)
    return t_lo + ((slot * 2**32 + r0) * R) // (n_slots * 2**32)


def stratum(t_lo, t_hi, slot, n_slots):
    """[lo, hi) that sample ``slot`` of ``n_slots`` lands in"""
    R = t_hi - t_lo
    return t_lo + (slot * R) // n_slots, t_lo - (-(slot + 1) * R) // n_slots


def continuous_t(r0, t_lo, t_hi, slot=None, n_slots=0):
    f = np.float32
    u = f(r0 >> 8) * f(2.0**-24)
    if slot is not None:
        u = f(f(slot) + u) / f(n_slots)
    return f(f(t_lo) + f(f(f(t_hi) - f(t_lo)) * u))


def compose(n, zc, z2, noise_offset, perturbation):
    """(n1, n2) from the three float32 draws: n [B,C,H,W], zc [B,C,1,1], z2 [B,C,H,W]; an option of 0 keeps the bits"""
    f = np.float32
    n1 = n if noise_offset == 0 else (n + (f(noise_offset) * zc).astype(f)).astype(f)
    n2 = n1 if perturbation == 0 else (n1 + (f(perturbation) * z2).astype(f)).astype(f)
    return n1, n2
