"""Seeded synthetic pileups of the shapes BASELINE.json names (recipe: SURVEY.md 8d).

Panel: UD ~ N(0, sigma_k) with column s.d. (7, 5, 3, 1.5, ...), mu ~ 2*Beta(0.8, 0.8)
clipped to [0.02, 1.98].  Per marker: AF = clamp(mu/2); intended genotype
g2 ~ Binom(2, AF), contaminant g1 ~ Binom(2, AF); depth ~ Poisson(mean_depth);
each read comes from the contaminant with probability alpha_true, carries the alt
allele with probability g/2, has Phred q ~ UniformInt[q_lo, q_hi], and is replaced by
one of the three other bases with probability 10^(-q/10); strand 50/50 ('.'/',' for
ref, upper/lower-case letter otherwise); quality character = q + 33.

Pure numpy, deterministic for a given seed; the same arrays feed the HIP path and
the oracle.  `write_files` emits a samtools-style pileup + .UD/.mu/.bed so the CLI and
file readers can be exercised on the same data.
"""
from __future__ import annotations

import numpy as np

from .api import PileupData

_SD = (7.0, 5.0, 3.0, 1.5, 1.0, 0.8, 0.6, 0.5, 0.4, 0.3)
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
_LOWER = np.frombuffer(b"acgt", dtype=np.uint8)


def make_pileup(num_marker, mean_depth=30.0, num_pc=4, alpha_true=0.05, seed=1, q_lo=20, q_hi=40,
                missing_frac=0.0):
    rng = np.random.default_rng(seed)
    M, k = int(num_marker), int(num_pc)
    sd = np.array([_SD[i] if i < len(_SD) else 0.3 for i in range(k)])
    ud = rng.normal(0.0, 1.0, size=(M, k)) * sd
    mu = np.clip(2.0 * rng.beta(0.8, 0.8, size=M), 0.02, 1.98)
    af = np.clip(mu / 2.0, 0.00005, 0.99995)
    g2 = rng.binomial(2, af)
    g1 = rng.binomial(2, af)
    depth = rng.poisson(mean_depth, size=M).astype(np.int64)
    if missing_frac > 0:
        depth[rng.random(M) < missing_frac] = 0
    ref_i = rng.integers(0, 4, size=M)
    alt_i = (ref_i + rng.integers(1, 4, size=M)) % 4
    read_off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(depth, out=read_off[1:])
    R = int(read_off[-1])
    mk = np.repeat(np.arange(M), depth)
    from_contam = rng.random(R) < alpha_true
    g = np.where(from_contam, g1[mk], g2[mk])
    is_alt = rng.random(R) < (g / 2.0)
    q = rng.integers(q_lo, q_hi + 1, size=R)
    err = rng.random(R) < np.power(10.0, -q / 10.0)
    true_base = np.where(is_alt, alt_i[mk], ref_i[mk])
    obs_base = np.where(err, (true_base + rng.integers(1, 4, size=R)) % 4, true_base)
    fwd = rng.random(R) < 0.5
    is_ref = obs_base == ref_i[mk]
    ch = np.where(fwd, _BASES[obs_base], _LOWER[obs_base])
    ch = np.where(is_ref, np.where(fwd, ord("."), ord(",")), ch).astype(np.uint8)
    quals = (q + 33).astype(np.uint8)
    alt_base = _BASES[alt_i]
    nsite = int((depth > 0).sum())
    avg = float(R) / nsite if nsite else float("nan")
    d = PileupData(k, ud, mu, read_off, ch, quals, alt_base, None, avg, 0.0, True,
                   dict(seed=seed, alpha_true=alpha_true, mean_depth=mean_depth,
                        ref_base=_BASES[ref_i]))
    return d


def with_sanity_stats(d: PileupData):
    """avgDepth/sdDepth as IsSanityCheckOK computes them (ContaminationEstimator.cpp:543-587),
    enabling the +-3sd depth filter."""
    depth = np.diff(d.read_off).astype(np.float64)
    present = depth > 0
    n = int(present.sum())
    avg = depth.sum() / n
    sd = float(np.sqrt((depth[present] ** 2).sum() / n - avg * avg))
    return PileupData(d.num_pc, d.ud, d.means, d.read_off, d.bases, d.quals, d.alt_base, d.known_af,
                      float(avg), sd, False, dict(d.meta))


def write_files(d: PileupData, prefix):
    """Write <prefix>.UD/.mu/.bed and <prefix>.pileup (6-column samtools pileup)."""
    M = d.num_marker
    ref = d.meta["ref_base"]
    with open(prefix + ".UD", "w") as f:
        for i in range(M):
            f.write("\t".join(repr(float(x)) for x in d.ud[i]) + "\n")
    with open(prefix + ".mu", "w") as f:
        for i in range(M):
            f.write("1:%d_%s/%s_rs%d\t%r\n" % (1000 + 10 * i, chr(ref[i]), chr(d.alt_base[i]), i,
                                                float(d.means[i])))
    with open(prefix + ".bed", "w") as f:
        for i in range(M):
            p = 1000 + 10 * i
            f.write("1\t%d\t%d\t%s\t%s\n" % (p - 1, p, chr(ref[i]), chr(d.alt_base[i])))
    bases = d.bases.tobytes().decode("latin-1")
    quals = d.quals.tobytes().decode("latin-1")
    with open(prefix + ".pileup", "w") as f:
        for i in range(M):
            b, e = int(d.read_off[i]), int(d.read_off[i + 1])
            if e == b:
                continue
            f.write("1\t%d\t%s\t%d\t%s\t%s\n" % (1000 + 10 * i, chr(ref[i]), e - b, bases[b:e], quals[b:e]))
    return prefix


def reads_on_panel(means, ref_char, alt_char, mean_depth=30.0, alpha_true=0.05, seed=1, q_lo=20, q_hi=40):
    """The read-drawing half of the recipe on a GIVEN panel (e.g. the reference's bundled
    1000g.phase3 panels: real mean genotypes, real ref/alt alleles -- first character of the
    .bed columns, like the reference reads them).  Genotypes ~ Binom(2, clamp(mu/2)) for both
    samples.  Returns (read_off, bases, quals): one pileup entry per panel row, in row order."""
    rng = np.random.default_rng(seed)
    mu = np.asarray(means, dtype=np.float64)
    M = mu.shape[0]
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    ref_i = np.array([code.get(int(c), 0) for c in np.asarray(ref_char, dtype=np.uint8)])
    alt_i = np.array([code.get(int(c), 1) for c in np.asarray(alt_char, dtype=np.uint8)])
    af = np.clip(mu / 2.0, 0.00005, 0.99995)
    g2 = rng.binomial(2, af)
    g1 = rng.binomial(2, af)
    return _draw_reads(rng, g1, g2, ref_i, alt_i, mean_depth, alpha_true, q_lo, q_hi)


def _draw_reads(rng, g1, g2, ref_i, alt_i, mean_depth, alpha_true, q_lo, q_hi):
    M = g2.shape[0]
    depth = rng.poisson(mean_depth, size=M).astype(np.int64)
    read_off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(depth, out=read_off[1:])
    R = int(read_off[-1])
    mk = np.repeat(np.arange(M), depth)
    g = np.where(rng.random(R) < alpha_true, g1[mk], g2[mk])
    is_alt = rng.random(R) < (g / 2.0)
    q = rng.integers(q_lo, q_hi + 1, size=R)
    err = rng.random(R) < np.power(10.0, -q / 10.0)
    true_base = np.where(is_alt, alt_i[mk], ref_i[mk])
    obs_base = np.where(err, (true_base + rng.integers(1, 4, size=R)) % 4, true_base)
    fwd = rng.random(R) < 0.5
    ch = np.where(fwd, _BASES[obs_base], _LOWER[obs_base])
    ch = np.where(obs_base == ref_i[mk], np.where(fwd, ord("."), ord(",")), ch).astype(np.uint8)
    return read_off, ch, (q + 33).astype(np.uint8)


def reads_from_genotypes(g_intended, g_contaminant, ref_char, alt_char, mean_depth=30.0, alpha_true=0.05, seed=1,
                         q_lo=20, q_hi=40):
    """reads_on_panel with EXPLICIT genotypes (0/1/2 per marker) for the intended sample and the contaminant, e.g.
    individuals drawn from the populations of write_structured_vcf."""
    rng = np.random.default_rng(seed)
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    ref_i = np.array([code.get(int(c), 0) for c in np.asarray(ref_char, dtype=np.uint8)])
    alt_i = np.array([code.get(int(c), 1) for c in np.asarray(alt_char, dtype=np.uint8)])
    return _draw_reads(rng, np.asarray(g_contaminant), np.asarray(g_intended), ref_i, alt_i, mean_depth, alpha_true,
                       q_lo, q_hi)


def write_structured_vcf(path, num_marker, num_sample, num_pop=3, fst=0.1, missing=0.02, seed=1, formats="mixed",
                         skipped_every=0, chroms=("1", "2", "3")):
    """A seeded reference-panel VCF with population structure (the Balding-Nichols model): ancestral allele
    frequencies p ~ U(0.05, 0.95), population frequencies ~ Beta(p (1 - F) / F, (1 - p)(1 - F) / F), samples dealt to
    the populations in turn, genotypes ~ Binom(2, p_pop).  formats="mixed" draws each marker's FORMAT from GT, PL, GL
    and GT:PL (PL/GL: 0 at the true genotype, 10-99 elsewhere); "GT" writes hard calls only.  A fraction `missing` of
    the values is "." (or "./." in GT).  skipped_every=k adds, after every k-th marker, a row the reader must skip
    (FILTER q10, a second ALT, an indel, chromosome X, in turn).  Written gzip'd when path ends in .gz.

    Returns dict(pop (population of each sample), freqs (num_pop x num_marker), ref, alt (uint8 per kept marker),
    chr, pos (per kept marker))."""
    import gzip
    rng = np.random.default_rng(seed)
    M, N = int(num_marker), int(num_sample)
    p = rng.uniform(0.05, 0.95, size=M)
    a = p * (1 - fst) / fst
    b = (1 - p) * (1 - fst) / fst
    freqs = np.clip(rng.beta(a[None, :].repeat(num_pop, 0), b[None, :].repeat(num_pop, 0)), 0.001, 0.999)
    pop = np.arange(N) % num_pop
    G = rng.binomial(2, freqs[pop].T)                       # M x N
    miss = rng.random((M, N)) < missing
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = bases[rng.integers(0, 4, size=M)]
    alt = bases[(np.searchsorted(bases, ref) + rng.integers(1, 4, size=M)) % 4]
    other = rng.integers(10, 100, size=(M, N, 3))
    fmt_names = ("GT", "PL", "GL", "GT:PL") if formats == "mixed" else (formats,)
    fmt_pick = rng.integers(0, len(fmt_names), size=M)
    gt_txt = np.array(["0/0", "0/1", "1/1"])
    per_chr = (M + len(chroms) - 1) // len(chroms)
    chr_of = [chroms[min(i // per_chr, len(chroms) - 1)] for i in range(M)]
    pos_of = np.zeros(M, dtype=np.int64)
    def opener(p, mode):
        return gzip.open(p, mode, compresslevel=1) if str(p).endswith(".gz") else open(p, mode)
    with opener(path, "wt") as f:
        f.write("##fileformat=VCFv4.1\n")
        f.write("##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n")
        f.write("##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype likelihoods\">\n")
        f.write("##FORMAT=<ID=GL,Number=G,Type=Float,Description=\"Log10-scaled genotype likelihoods\">\n")
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
                "\t".join("S%05d" % j for j in range(N)) + "\n")
        pos = 1000
        prev_chr = None
        nskip = 0
        for i in range(M):
            if chr_of[i] != prev_chr:
                pos, prev_chr = 1000, chr_of[i]
            pos += 10
            pos_of[i] = pos
            fmt = fmt_names[fmt_pick[i]]
            g = G[i]
            ph = other[i].copy()
            ph[np.arange(N), g] = 0
            pl = ["%d,%d,%d" % tuple(r) for r in ph]
            if fmt == "GT":
                vals = list(gt_txt[g])
            elif fmt == "PL":
                vals = pl
            elif fmt == "GL":
                vals = ["%.1f,%.1f,%.1f" % tuple(-r / 10.0) for r in ph]
            else:
                vals = ["%s:%s" % (gt_txt[g[j]], pl[j]) for j in range(N)]
            for j in np.nonzero(miss[i])[0]:
                vals[j] = "./." if fmt == "GT" else "."
            f.write("%s\t%d\t.\t%s\t%s\t.\tPASS\t.\t%s\t%s\n" % (chr_of[i], pos, chr(ref[i]), chr(alt[i]), fmt,
                                                               "\t".join(vals)))
            if skipped_every and (i + 1) % skipped_every == 0:
                pos += 5
                kind = nskip % 4
                nskip += 1
                c, r_, a_, flt = chr_of[i], chr(ref[i]), chr(alt[i]), "PASS"
                if kind == 0:
                    flt = "q10"
                elif kind == 1:
                    a_ = a_ + ",T" if a_ != "T" else a_ + ",G"
                elif kind == 2:
                    r_ = r_ + "AC"
                else:
                    c = "X"
                f.write("%s\t%d\t.\t%s\t%s\t.\t%s\t.\tGT\t%s\n" % (c, pos, r_, a_, flt, "\t".join(gt_txt[g])))
    return dict(pop=pop, freqs=freqs, ref=ref, alt=alt, chr=chr_of, pos=pos_of, genotypes=np.where(miss, -1, G))


def read_bed_rows(bed_path):
    """(chr, pos, first char of ref, first char of alt) per row of a .bed (plain or gzip'd)."""
    import gzip
    raw = open(bed_path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    chrs, poss, refs, alts = [], [], [], []
    for line in raw.decode("latin-1").split("\n"):
        tok = line.split()
        if len(tok) < 5:
            continue
        chrs.append(tok[0]); poss.append(int(tok[2])); refs.append(ord(tok[3][0])); alts.append(ord(tok[4][0]))
    return chrs, np.array(poss), np.array(refs, dtype=np.uint8), np.array(alts, dtype=np.uint8)


def read_mu_column(mu_path):
    import gzip
    raw = open(mu_path, "rb").read()
    if raw[:2] == b"\x1f\x8b":
        raw = gzip.decompress(raw)
    return np.array([float(line.split()[1]) for line in raw.decode("latin-1").split("\n") if line.strip()])


def write_pileup_text(path, chrs, poss, ref_char, read_off, bases, quals):
    """6-column samtools pileup for the drawn reads, one line per covered panel row."""
    b = np.asarray(bases, dtype=np.uint8).tobytes().decode("latin-1")
    q = np.asarray(quals, dtype=np.uint8).tobytes().decode("latin-1")
    with open(path, "w") as f:
        for i in range(len(chrs)):
            lo, hi = int(read_off[i]), int(read_off[i + 1])
            if hi > lo:
                f.write("%s\t%d\t%s\t%d\t%s\t%s\n" % (chrs[i], int(poss[i]), chr(int(ref_char[i])), hi - lo, b[lo:hi], q[lo:hi]))
    return path


def real_panel_sample(svd_prefix, pileup_path, mean_depth=30.0, alpha_true=0.05, seed=1):
    """Draws reads on the panel behind `svd_prefix` (.mu/.bed) and writes them as a text pileup."""
    chrs, poss, refs, alts = read_bed_rows(svd_prefix + ".bed")
    mu = read_mu_column(svd_prefix + ".mu")
    off, b, q = reads_on_panel(mu, refs, alts, mean_depth, alpha_true, seed)
    return write_pileup_text(pileup_path, chrs, poss, refs, off, b, q)


def write_known_af(svd_prefix, path, seed=1):
    """A --KnownAF file for the panel behind `svd_prefix` (.bed/.mu): one `chr start end ref alt af` row per panel
    row, af = clamp(mu / 2 + N(0, 0.02)) -- seeded, so a fixture recipe and its tests write the same file."""
    chrs, poss, refs, alts = read_bed_rows(svd_prefix + ".bed")
    mu = read_mu_column(svd_prefix + ".mu")
    rng = np.random.default_rng(seed)
    af = np.clip(mu / 2.0 + rng.normal(0.0, 0.02, size=mu.shape[0]), 0.001, 0.999)
    with open(path, "w") as f:
        for i in range(len(chrs)):
            f.write("%s\t%d\t%d\t%s\t%s\t%r\n" % (chrs[i], int(poss[i]) - 1, int(poss[i]), chr(int(refs[i])),
                                                  chr(int(alts[i])), float(af[i])))
    return path
