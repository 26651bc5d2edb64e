// baq_core.h -- base alignment quality and the mapping-quality cap, written once for host and device
// as bgzf_inflate_core.h is: the banded profile HMM (the reference's samtools/kprobaln.c: kpa_glocal), the wrapper that picks
// the window and folds the posteriors into the qualities (samtools/bam_md.c: bam_prob_realn_core) and the CIGAR walk of
// the cap (bam_cap_mapQ), restated from reading them.  No HIP header: tests/baq_check_main.cpp compiles this for the host
// alone.
//
// What decides the bits: IEEE double in the reference's order of operations with contraction OFF (the pragma below and
// -ffp-contract=off on the units that include this), the gap parameters in single precision, EM = .33333333333, the
// quality table float(pow(10, -i/10.)) from the host's libm, every cell outside the band read as zero from a zeroed row
// of bw2*3 + 6 doubles, the row sum and the deletion chain sequential in k, the MAP with a strict > in ascending k (M
// before I).  The device never calls log: 1 - max/sum is quantised by a search in thresholds the host found with its
// own libm (Tables::thresh below, built in baq_host.cpp), so the device's quality IS the host libm's.
//
// One record is worked on by `lanes` cooperating lanes (1 on the host, 16 on the device).  M and I of a row go a cell per
// lane; the deletion chain, the row sum and the MAP are lane 0's, in the reference's order.  Every lane of a workgroup
// calls the functions below with the same `rows` (the largest l_query among the workgroup's records), so that `sync`
// (a workgroup barrier on the device, nothing on the host) is reached by all of them alike.
#ifndef VB2_BAQ_CORE_H_
#define VB2_BAQ_CORE_H_

#include <cstdint>

#if defined(__HIPCC__)
#define VB2_BAQ_HD __host__ __device__
#else
#define VB2_BAQ_HD
#endif

#pragma STDC FP_CONTRACT OFF

namespace vb2 {
namespace baq {

// ---- outcome of a record (vb2_baq_records' code) ----
enum Outcome : uint8_t {
    kRealigned = 0,      // the HMM ran and its qualities were applied
    kAlone = 1,          // left alone by rule: unmapped, no bases, qualities 0xFF, an N operation, a ZQ tag
    kTagApplied = 2,     // a BQ tag was there (and no redo): applied, no HMM
    kNoReference = 3,    // the FASTA lacks the sequence: neither BAQ nor the cap
    kOutside = 4,        // pos >= the sequence's length: the read is dropped
    kCapDropped = 5,     // the cap's t exceeded the threshold: the read is dropped
    kNotAsked = 6        // BAQ is off in the options (the cap may still have run)
};

constexpr int kRowPad = 6;
VB2_BAQ_HD inline int row_doubles(int bw) { return (bw * 2 + 1) * 3 + kRowPad; }
VB2_BAQ_HD inline int band_of(int l_ref, int l_query, int conf_bw)
{
    int bw = l_ref > l_query ? l_ref : l_query;
    if (bw > conf_bw) bw = conf_bw;
    const int d = l_ref > l_query ? l_ref - l_query : l_query - l_ref;
    if (bw < d) bw = d;
    return bw;
}
// the workspace of one record in bytes: forward matrix (l_query + 1 rows), two backward rows, the scaling factors, and per
// base a state word and a quality byte (rounded to 8)
VB2_BAQ_HD inline uint64_t work_bytes(int l_ref, int l_query, int conf_bw)
{
    const uint64_t w = (uint64_t)row_doubles(band_of(l_ref, l_query, conf_bw));
    return ((uint64_t)l_query + 3) * w * 8 + ((uint64_t)l_query + 2) * 8 + (((uint64_t)l_query * 5 + 7) & ~7ull);
}

struct Work {
    double* f;           // (l_query + 1) rows
    double* b;           // 2 rows
    double* s;           // l_query + 2
    int32_t* state;      // l_query
    uint8_t* q;          // l_query
};
VB2_BAQ_HD inline Work carve(void* base, int l_ref, int l_query, int conf_bw)
{
    const uint64_t w = (uint64_t)row_doubles(band_of(l_ref, l_query, conf_bw));
    Work k;
    k.f = static_cast<double*>(base);
    k.b = k.f + ((uint64_t)l_query + 1) * w;
    k.s = k.b + 2 * w;
    k.state = reinterpret_cast<int32_t*>(k.s + (uint64_t)l_query + 2);
    k.q = reinterpret_cast<uint8_t*>(k.state + l_query);
    return k;
}

// the tables the host builds once per process with its libm
struct Tables {
    float qual2prob[256];          // float(pow(10, -i/10.))
    double thresh[101];            // thresh[j]: the largest double z with (int)(-4.343*log(z) + .499) >= j + 1
};

// (int)(-4.343*log(z) + .499) for 0 < z: how many thresholds z does not exceed.  101 stands for "above 100".
VB2_BAQ_HD inline int quantise(const double* thresh, double z)
{
    int a = 0, b = 101;            // thresh is descending: find the number of j with z <= thresh[j]
    while (a < b) {
        const int mid = (a + b) >> 1;
        if (z <= thresh[mid]) a = mid + 1;
        else b = mid;
    }
    return a;
}

VB2_BAQ_HD inline int nt16_int(int c)        // htslib's seq_nt16_int: A C G T -> 0..3, every other code 4
{
    return c == 1 ? 0 : c == 2 ? 1 : c == 4 ? 2 : c == 8 ? 3 : 4;
}

// The query of the HMM: codes 0..4 one per byte (codes != null), or a BAM record's packed 4-bit codes; qualities one per
// byte, after the Illumina-1.3 shift where asked for.
struct Query {
    const uint8_t* codes;
    const uint8_t* packed;
    const uint8_t* qual;
    int illumina;
};
VB2_BAQ_HD inline int query_code(const Query& q, int i)      // i 0-based
{
    if (q.codes) return q.codes[i];
    return nt16_int((q.packed[i >> 1] >> ((i & 1) ? 0 : 4)) & 15);
}
VB2_BAQ_HD inline int shifted(int q, int illumina) { return illumina ? (q > 31 ? q - 31 : 0) : q; }
VB2_BAQ_HD inline int query_qual(const Query& q, int i) { return shifted(q.qual[i], q.illumina); }

// The reference of the HMM: codes 0..4 one per byte (nt16 == 0), or nt16 codes one per byte (a span of the FASTA).
struct Ref {
    const uint8_t* p;
    int nt16;
};
VB2_BAQ_HD inline int ref_code(const Ref& r, int k) { return r.nt16 ? nt16_int(r.p[k]) : r.p[k]; }      // k 0-based

#define VB2_BAQ_SET_U(u, b, i, k) { int x_ = (i) - (b); x_ = x_ > 0 ? x_ : 0; (u) = ((k) - x_ + 1) * 3; }

// kpa_glocal with state and q asked for.  l_query may be 0 (a lane group without a record: it only keeps the barriers);
// l_ref <= 0 leaves state and q zero, as the reference's early return leaves its caller's calloc'ed arrays.
// Returns (to lane 0) the number of undefined rows: rows whose posterior sum is not positive or whose 1 - max/sum is not,
// where the reference converts a NaN or an infinity to int.  Their quality is 0.
template <class Sync>
VB2_BAQ_HD inline int glocal(const Ref& ref, int l_ref, const Query& qy, int l_query, int conf_bw, const Tables* tb, const Work& w,
                             int lane, int lanes, int rows, Sync sync)
{
    const double EI = .25, EM = .33333333333;
    const float cd = 0.001f, ce = 0.1f;
    const bool run = l_query > 0 && l_ref > 0;
    const int lq = run ? l_query : 0;
    const int bw = band_of(l_ref, l_query > 0 ? l_query : 1, conf_bw), bw2 = bw * 2 + 1, W = bw2 * 3 + kRowPad;
    int undefined = 0;
    for (int i = lane; i < l_query; i += lanes) {
        w.state[i] = 0;
        w.q[i] = 0;
    }
    if (run) {
        const int64_t nf = (int64_t)(lq + 1) * W + 2 * W + lq + 2;      // f, b and s are contiguous
        for (int64_t j = lane; j < nf; j += lanes) w.f[j] = 0.;
    }
    sync();
    double m[9], sM, sI, bM, bI;
    sM = sI = 1. / (2 * (run ? l_query : 1) + 2);
    m[0] = (1 - cd - cd) * (1 - sM); m[1] = m[2] = cd * (1 - sM);
    m[3] = (1 - ce) * (1 - sI); m[4] = ce * (1 - sI); m[5] = 0.;
    m[6] = 1 - ce; m[7] = 0.; m[8] = ce;
    bM = (1 - cd) / (run ? l_ref : 1); bI = cd / (run ? l_ref : 1);
    // ---- forward ----
    if (run && lane == 0) {
        int k;
        VB2_BAQ_SET_U(k, bw, 0, 0);
        w.f[k] = w.s[0] = 1.;
    }
    {   // f[1]
        const int end = l_ref < bw + 1 ? l_ref : bw + 1;
        double* fi = w.f + W;
        if (run) {
            const int q1 = query_code(qy, 0);
            const double ql = tb->qual2prob[query_qual(qy, 0)];
            for (int k = 1 + lane; k <= end; k += lanes) {
                const int rk = ref_code(ref, k - 1);
                const double e = (rk > 3 || q1 > 3) ? 1. : rk == q1 ? 1. - ql : ql * EM;
                int u;
                VB2_BAQ_SET_U(u, bw, 1, k);
                fi[u + 0] = e * bM;
                fi[u + 1] = EI * bI;
            }
        }
        sync();
        if (run && lane == 0) {
            double sum = 0.;
            for (int k = 1; k <= end; ++k) {
                int u;
                VB2_BAQ_SET_U(u, bw, 1, k);
                sum += fi[u] + fi[u + 1];
            }
            w.s[1] = sum;
        }
        sync();
        if (run) {
            const double sum = w.s[1];
            for (int k = 1 + lane; k <= end; k += lanes) {
                int u;
                VB2_BAQ_SET_U(u, bw, 1, k);
                fi[u] /= sum; fi[u + 1] /= sum; fi[u + 2] /= sum;
            }
        }
        sync();
    }
    for (int i = 2; i <= rows; ++i) {
        const bool on = i <= lq;
        double* fi = w.f + (int64_t)(on ? i : 0) * W;
        const double* fi1 = w.f + (int64_t)(on ? i - 1 : 0) * W;
        int beg = 1, end = l_ref, x;
        x = i - bw; beg = beg > x ? beg : x;
        x = i + bw; end = end < x ? end : x;
        if (on) {
            const double qli = tb->qual2prob[query_qual(qy, i - 1)];
            const int qyi = query_code(qy, i - 1);
            for (int k = beg + lane; k <= end; k += lanes) {
                int u, v11, v10;
                const int rk = ref_code(ref, k - 1);
                const double e = (rk > 3 || qyi > 3) ? 1. : rk == qyi ? 1. - qli : qli * EM;
                VB2_BAQ_SET_U(u, bw, i, k); VB2_BAQ_SET_U(v11, bw, i - 1, k - 1); VB2_BAQ_SET_U(v10, bw, i - 1, k);
                fi[u + 0] = e * (m[0] * fi1[v11 + 0] + m[3] * fi1[v11 + 1] + m[6] * fi1[v11 + 2]);
                fi[u + 1] = EI * (m[1] * fi1[v10 + 0] + m[4] * fi1[v10 + 1]);
            }
        }
        sync();
        if (on && lane == 0) {
            double sum = 0.;
            for (int k = beg; k <= end; ++k) {
                int u, v01;
                VB2_BAQ_SET_U(u, bw, i, k); VB2_BAQ_SET_U(v01, bw, i, k - 1);
                fi[u + 2] = m[2] * fi[v01 + 0] + m[8] * fi[v01 + 2];
                sum += fi[u] + fi[u + 1] + fi[u + 2];
            }
            w.s[i] = sum;
        }
        sync();
        if (on) {
            const double r = 1. / w.s[i];
            for (int k = beg + lane; k <= end; k += lanes) {
                int u;
                VB2_BAQ_SET_U(u, bw, i, k);
                fi[u] *= r; fi[u + 1] *= r; fi[u + 2] *= r;
            }
        }
        sync();
    }
    if (run && lane == 0) {      // s[l_query + 1]
        double sum = 0.;
        const double* fl = w.f + (int64_t)lq * W;
        for (int k = 1; k <= l_ref; ++k) {
            int u;
            VB2_BAQ_SET_U(u, bw, lq, k);
            if (u < 3 || u >= bw2 * 3 + 3) continue;
            sum += fl[u + 0] * sM + fl[u + 1] * sI;
        }
        w.s[lq + 1] = sum;
    }
    sync();
    // ---- backward, two rows, the MAP of a row as soon as the row is there ----
    for (int i = rows; i >= 1; --i) {
        const bool on = i <= lq;
        double* bi = w.b + (on ? (i & 1) : 0) * W;
        const double* bi1 = w.b + (on ? ((i + 1) & 1) : 0) * W;
        const double* fi = w.f + (int64_t)(on ? i : 0) * W;
        int beg = 1, end = l_ref, x;
        x = i - bw; beg = beg > x ? beg : x;
        x = i + bw; end = end < x ? end : x;
        if (on && i < lq)
            for (int j = lane; j < W; j += lanes) bi[j] = 0.;
        sync();
        if (on && i == lq) {
            const double vM = sM / w.s[lq] / w.s[lq + 1], vI = sI / w.s[lq] / w.s[lq + 1];
            for (int k = 1 + lane; k <= l_ref; k += lanes) {
                int u;
                VB2_BAQ_SET_U(u, bw, lq, k);
                if (u < 3 || u >= bw2 * 3 + 3) continue;
                bi[u + 0] = vM; bi[u + 1] = vI;
            }
        } else if (on) {
            const double qli1 = tb->qual2prob[query_qual(qy, i)];
            const int qyi1 = query_code(qy, i);
            for (int k = beg + lane; k <= end; k += lanes) {
                int u, v11, v10;
                VB2_BAQ_SET_U(u, bw, i, k); VB2_BAQ_SET_U(v11, bw, i + 1, k + 1); VB2_BAQ_SET_U(v10, bw, i + 1, k);
                double e0 = 0;
                if (k < l_ref) {
                    const int rk = ref_code(ref, k);
                    e0 = (rk > 3 || qyi1 > 3) ? 1. : rk == qyi1 ? 1. - qli1 : qli1 * EM;
                }
                const double e = e0 * bi1[v11];
                bi[u + 0] = e * m[0] + EI * m[1] * bi1[v10 + 1];      // (+ m[2] * D of k + 1: lane 0's chain below)
                bi[u + 1] = e * m[3] + EI * m[4] * bi1[v10 + 1];
                bi[u + 2] = e * m[6];
            }
        }
        sync();
        if (on && i < lq && lane == 0) {
            const double y = i > 1;
            for (int k = end; k >= beg; --k) {
                int u, v01;
                VB2_BAQ_SET_U(u, bw, i, k); VB2_BAQ_SET_U(v01, bw, i, k + 1);
                const double dn = bi[v01 + 2];
                bi[u + 0] = bi[u + 0] + m[2] * dn;
                bi[u + 2] = (bi[u + 2] + m[8] * dn) * y;
            }
        }
        sync();
        if (on && i < lq) {
            const double y = 1. / w.s[i];
            for (int k = beg + lane; k <= end; k += lanes) {
                int u;
                VB2_BAQ_SET_U(u, bw, i, k);
                bi[u] *= y; bi[u + 1] *= y; bi[u + 2] *= y;
            }
        }
        sync();
        if (on && lane == 0) {      // MAP of row i
            double sum = 0., max = 0.;
            int max_k = -1;
            for (int k = beg; k <= end; ++k) {
                int u;
                double z;
                VB2_BAQ_SET_U(u, bw, i, k);
                z = fi[u + 0] * bi[u + 0]; if (z > max) max = z, max_k = (int)((uint32_t)(k - 1) << 2 | 0u); sum += z;
                z = fi[u + 1] * bi[u + 1]; if (z > max) max = z, max_k = (int)((uint32_t)(k - 1) << 2 | 1u); sum += z;
            }
            w.state[i - 1] = max_k;
            int qv = 0;
            if (sum > 0.) {
                max /= sum;
                const double z = 1. - max;
                if (z > 0.) {
                    const int kq = quantise(tb->thresh, z);
                    qv = kq > 100 ? 99 : kq;
                } else {
                    ++undefined;
                }
            } else {
                ++undefined;
            }
            w.q[i - 1] = (uint8_t)qv;
        }
    }
    sync();
    return undefined;
}

// ---- the wrapper's plan: what the CIGAR says (bam_md.c:219-269), done once per record on the host ----
struct Plan {
    int32_t xb, xe;       // the reference window [xb, xe), already cut at the sequence's end
    int32_t bw;           // conf.bw
    uint8_t hmm;          // 1: run the HMM; 0: the outcome below is final
    uint8_t outcome;
};
VB2_BAQ_HD inline uint32_t rd32u(const uint8_t* p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// cigar: n_cigar little-endian words, unaligned.  first_qual: the first quality AFTER the Illumina shift.
VB2_BAQ_HD inline Plan plan_record(int32_t pos, int32_t l_qseq, uint32_t flag, const uint8_t* cigar, uint32_t n_cigar, int first_qual,
                                   bool has_bq, bool has_zq, bool redo, int64_t ref_len)
{
    Plan p{0, 0, 7, 0, kAlone};
    if ((flag & 4) || l_qseq == 0 || first_qual == 0xFF) return p;
    if (has_bq && redo) has_bq = false;
    if (has_bq && has_zq) has_zq = false;
    if (has_zq) return p;
    if (has_bq) {
        p.outcome = kTagApplied;
        return p;
    }
    int64_t x = pos, y = 0, yb = -1, ye = -1, xb = -1, xe = -1;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = rd32u(cigar + 4ull * k), op = c & 15;
        const int64_t l = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (yb < 0) yb = y;
            if (xb < 0) xb = x;
            ye = y + l; xe = x + l;
            x += l; y += l;
        } else if (op == 4 || op == 1) {
            y += l;
        } else if (op == 2) {
            x += l;
        } else if (op == 3) {
            return p;
        }
    }
    // a CIGAR whose query length is not the record's would make the reference read past its arrays: left alone
    if (y != l_qseq || x > 0x7fffffff) return p;
    int64_t bw = 7;
    int64_t d = (xe - xb) - (ye - yb);
    if (d < 0) d = -d;
    if (d > bw) bw = d + 3;
    xb -= yb + bw / 2; if (xb < 0) xb = 0;
    xe += l_qseq - ye + bw / 2;
    if (xe - xb - l_qseq > bw) {
        const int64_t t = (xe - xb - l_qseq - bw) / 2;
        xb += t;
        xe -= (xe - xb - l_qseq - bw) / 2;      // (the reference reads the moved xb here)
    }
    if (xe > ref_len) xe = ref_len;
    if (xe < xb) xe = xb;                       // (an empty window: the HMM returns at once, state and q stay zero)
    p.xb = (int32_t)xb;
    p.xe = (int32_t)xe;
    p.bw = (int32_t)bw;
    p.hmm = 1;
    p.outcome = kRealigned;
    return p;
}

// The qualities before BAQ: out[i] = the record's, shifted where asked for.
VB2_BAQ_HD inline void copy_quals(const uint8_t* qual, int l_qseq, int illumina, uint8_t* out, int lane, int lanes)
{
    for (int i = lane; i < l_qseq; i += lanes) out[i] = (uint8_t)shifted(qual[i], illumina);
}
// A BQ tag applied (bam_md.c:236-239), on out[] as copy_quals left it
VB2_BAQ_HD inline void apply_bq_tag(const uint8_t* bq, int l_qseq, uint8_t* out, int lane, int lanes)
{
    for (int i = lane; i < l_qseq; i += lanes) {
        const int q = out[i], b = bq[i];
        out[i] = (uint8_t)(q + 64 < b ? 0 : q - (b - 64));
    }
}

// The extended block and the final subtraction (bam_md.c:298-320) by ONE lane, on out[] as copy_quals left it; state and q
// from glocal.  w.q is used up.
VB2_BAQ_HD inline void extend_apply(int32_t pos, int32_t l_qseq, const uint8_t* cigar, uint32_t n_cigar, int32_t xb, const Work& w,
                                    uint8_t* out)
{
    // bq[] of the reference starts as a copy of the qualities and is replaced inside match operations only: a base
    // of a soft clip or an insertion keeps its quality, which 0xFF stands for here (no quality exceeds it)
    int64_t x = pos, y = 0;
    uint8_t* bq = w.q;
    uint8_t* left = reinterpret_cast<uint8_t*>(w.state);      // (the states are used up by pass 1, their bytes serve pass 2)
    {   // pass 1: the folded posterior of every base
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t c = rd32u(cigar + 4ull * k), op = c & 15;
            const int64_t l = c >> 4;
            if (op == 0 || op == 7 || op == 8) {
                for (int64_t i = y; i < y + l; ++i) {
                    const int32_t st = w.state[i];
                    bq[i] = ((st & 3) != 0 || (int64_t)(st >> 2) != x - xb + (i - y)) ? (uint8_t)0 : bq[i];
                }
                x += l; y += l;
            } else if (op == 4 || op == 1) {
                for (int64_t i = y; i < y + l; ++i) bq[i] = 0xFF;
                y += l;
            } else if (op == 2) {
                x += l;
            }
        }
    }
    y = 0;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = rd32u(cigar + 4ull * k), op = c & 15;
        const int64_t l = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            if (l > 0) {
                left[y] = bq[y];
                for (int64_t i = y + 1; i < y + l; ++i) left[i] = bq[i] > left[i - 1] ? bq[i] : left[i - 1];
                uint8_t r = bq[y + l - 1];
                for (int64_t i = y + l - 1; i >= y; --i) {
                    r = bq[i] > r ? bq[i] : r;
                    bq[i] = left[i] < r ? left[i] : r;
                }
            }
            y += l;
        } else if (op == 4 || op == 1) {
            y += l;
        }
    }
    for (int32_t i = 0; i < l_qseq; ++i) {
        const int q = out[i], b = bq[i];
        const int t = 64 + (q <= b ? 0 : q - b);      // the BQ byte
        out[i] = (uint8_t)(q - (t - 64));
    }
}

// ---- the cap's CIGAR walk (bam_md.c:170-201) by one lane: mm, q, len, clip_q.  ref: nt16 codes, ref[0] is position
// ref_beg; positions at or behind ref_len end the walk as the reference's "out of bounds" does. ----
VB2_BAQ_HD inline void cap_walk(int32_t pos, const uint8_t* cigar, uint32_t n_cigar, const uint8_t* packed, const uint8_t* qual,
                                int32_t l_qseq, const uint8_t* ref, int64_t ref_beg, int64_t ref_len, int32_t out[4])
{
    int32_t mm = 0, q = 0, len = 0, clip_q = 0;
    int64_t x = pos, y = 0;
    for (uint32_t i = 0; i < n_cigar; ++i) {
        const uint32_t c = rd32u(cigar + 4ull * i), op = c & 15;
        const int64_t l = c >> 4;
        if (op == 0 || op == 7 || op == 8) {
            int64_t j;
            for (j = 0; j < l; ++j) {
                const int64_t z = y + j;
                if (x + j >= ref_len || z >= l_qseq) break;
                const int c1 = (packed[z >> 1] >> ((z & 1) ? 0 : 4)) & 15, c2 = ref[x + j - ref_beg];
                if (c2 != 15 && c1 != 15 && qual[z] >= 13) {
                    ++len;
                    if (c1 && c1 != c2) {
                        ++mm;
                        q += qual[z] > 33 ? 33 : qual[z];
                    }
                }
            }
            if (j < l) break;
            x += l; y += l; len += (int32_t)l;
        } else if (op == 2) {
            if (l > 0 && x + l > ref_len) break;
            x += l;
        } else if (op == 4) {
            for (int64_t j = 0; j < l && y + j < l_qseq; ++j) clip_q += qual[y + j];
            y += l;
        } else if (op == 5) {
            clip_q += 13 * (int32_t)l;
        } else if (op == 1) {
            y += l;
        } else if (op == 3) {
            x += l;
        }
    }
    out[0] = mm; out[1] = q; out[2] = len; out[3] = clip_q;
}

}  // namespace baq
}  // namespace vb2

#endif
