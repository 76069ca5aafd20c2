#!/usr/bin/env python3
"""Golden data for tests/test_oracle_vs_reference.py, computed in the build container with the reference's own
kappa sources (oracle/_ref), so that those tests run wherever the repository is checked out:

  oracle_vs_reference.npz
      bessel_z, bessel        -- 1200 random arguments (seed 1, four scales) and the reference's Bessel values
      kappa_ij, kappa_w, kappa -- 120 random (i, j, omega) on the N=96 tokamak grid of the test (seed 2) and the
                                  reference's kappa(0, eta_i, eta_j, omega)
      M_n48                   -- the whole tokamak matrix, N=48, omega = -0.8+0.25i
      M_stell_n12             -- the whole stellarator matrix, N=12 (dim 24), omega = -0.9+0.4i

The sampling is the test's own; the test regenerates the inputs and checks them against the stored ones.

Run:  python tests/golden/make_golden_oracle_vs_reference.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.binding import Oracle, Reference, example_stellarator, example_tokamak  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ref, orc = Reference(), Oracle()

rng = np.random.default_rng(1)
bz = np.array([complex(*(rng.normal(size=2) * s)) for s in (0.05, 1.0, 8.0, 40.0) for _ in range(300)])
bessel = np.array([ref.bessel(z) for z in bz])

d = example_tokamak(npoints=96, omega_d_coeff=0.71, theta=0.2, epsilon_r=0.05)
ref.open_dict(d)
p = orc.params(d)
eta, _ = orc.grid(p.length, p.npoints)
rng = np.random.default_rng(2)
ij, kw = [], []
for _ in range(120):
    i = int(rng.integers(0, 95))
    j = int(rng.integers(i + 1, 96))
    ij.append((i, j))
    kw.append(complex(rng.uniform(-1.2, 1.2), rng.uniform(-0.3, 0.5)))
kappa = np.array([ref.kappa(0, eta[i], eta[j], w) for (i, j), w in zip(ij, kw)])

ref.open_dict(example_tokamak(npoints=48))
M48 = ref.assemble(48, -0.8 + 0.25j)
ref.open_dict(example_stellarator(npoints=12))
Ms = ref.assemble(24, -0.9 + 0.4j)

np.savez_compressed(os.path.join(OUT, "oracle_vs_reference.npz"), bessel_z=bz, bessel=bessel,
                    kappa_ij=np.array(ij, dtype=np.int64), kappa_w=np.array(kw), kappa=kappa,
                    M_n48=M48, M_stell_n12=Ms)
print("wrote oracle_vs_reference.npz")
