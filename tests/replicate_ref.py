"""Shared by the replicate tests: the reference for a weighted log-likelihood is the pinned oracle on the EXPANDED input --
marker i's pileup row and panel row repeated w_i times and dropped at 0, the depth statistics and the sanity flag carried
over unchanged (so the +-3 sd filter decides identically).  That value is sum_i w_i log L_i by construction."""
import numpy as np

import verifybamid_amd as vb
from oracle.bridge import oracle_data


def expand(d, w):
    """PileupData with marker i repeated w[i] times."""
    w = np.asarray(w, dtype=np.int64)
    assert w.shape == (d.num_marker,)
    rep = np.repeat(np.arange(d.num_marker), w)
    depth = np.diff(d.read_off)
    off = np.zeros(rep.shape[0] + 1, dtype=np.int64)
    np.cumsum(depth[rep], out=off[1:])
    # read j of expanded row e is read read_off[rep[e]] + j of the input
    idx = np.repeat(d.read_off[:-1][rep] - off[:-1], depth[rep]) + np.arange(int(off[-1]), dtype=np.int64)
    return vb.PileupData(d.num_pc, d.ud[rep], d.means[rep], off, d.bases[idx], d.quals[idx], d.alt_base[rep],
                         None if d.known_af is None else d.known_af[rep], d.avg_depth, d.sd_depth, d.sanity_disabled,
                         dict(d.meta))


class ExpandedOracle:
    """The oracle on the expanded input of each weight row, built once per row."""

    def __init__(self, d, weights):
        self.d = d
        self.weights = np.atleast_2d(np.asarray(weights))
        self._od = {}

    def data(self, r):
        if r not in self._od:
            self._od[r] = oracle_data(expand(self.d, self.weights[r])) if self.weights[r].any() else None
        return self._od[r]

    def llk(self, r, pc1, pc2, alpha):
        od = self.data(r)
        return 0.0 if od is None else od.llk(pc1, pc2, alpha)

    def evaluate(self, num_point, pc1, pc2, alpha):
        """The evaluator of replicates_with_evaluator: every replicate's points, concatenated in replicate order."""
        out, p = [], 0
        for r, n in enumerate(num_point):
            for _ in range(int(n)):
                out.append(self.llk(r, pc1[p], pc2[p], alpha[p]))
                p += 1
        return np.array(out)


def splitmix_draws(seed, r, num_marker):
    """A Python restatement of vb2_bootstrap_weights' generator: replicate r's num_marker marker indices."""
    mask = (1 << 64) - 1
    s = ((int(seed) << 32) ^ ((0x5851f42d4c957f2d * (r + 1)) & mask)) & mask
    out = []
    for _ in range(num_marker):
        s = (s + 0x9e3779b97f4a7c15) & mask
        z = s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & mask
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & mask
        z = z ^ (z >> 31)
        out.append((z * num_marker) >> 64)
    return out


def jackknife_numpy(m, theta_hat, theta_without):
    """The delete-m_j jackknife of Busing, Meijer and van der Leeden (1999), restated: blocks with m = 0 left out."""
    m = np.asarray(m, dtype=np.float64)
    t = np.asarray(theta_without, dtype=np.float64)
    keep = m > 0
    m, t = m[keep], t[keep]
    g, n = len(m), m.sum()
    h = n / m
    est = g * theta_hat - np.sum((1 - m / n) * t)
    tau = h * theta_hat - (h - 1) * t
    se = np.sqrt(np.sum((tau - est) ** 2 / (h - 1)) / g)
    return est, se
