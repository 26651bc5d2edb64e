// baq_host.cpp -- see baq_host.h.  Built with -ffp-contract=off like every unit that includes baq_core.h.
#include "baq_host.h"
#include "host_clock.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

namespace vb2 {
namespace baq {

namespace {

struct NoSync {
    void operator()() const {}
};

inline uint32_t le32(const uint8_t* p) { return rd32u(p); }

// what one record needs of its sequence: the HMM's window and the cap's walk
struct Need {
    Plan plan;
    int64_t lo = 0, hi = 0;      // empty when lo >= hi
};

Need need_of(const bamio::Chunk& ch, const bamio::RecordDesc& d, const Options& opt, int64_t ref_len)
{
    Need n;
    n.plan = Plan{0, 0, 7, 0, kNotAsked};
    if (ref_len < 0 || d.pos >= ref_len) return n;
    const uint8_t* rec = ch.bytes.data() + d.data;
    const uint8_t* cig = rec + d.l_read_name;
    const uint8_t* qual = cig + 4ull * d.n_cigar + ((uint64_t)d.l_seq + 1) / 2;
    int64_t lo = d.pos, hi = d.pos;
    if (opt.cap_on()) {
        int64_t rlen = 0;
        for (uint32_t k = 0; k < d.n_cigar; ++k) {
            const uint32_t c = le32(cig + 4ull * k), op = c & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += c >> 4;
        }
        hi = std::min<int64_t>(d.pos + rlen, ref_len);
    }
    if (opt.realn) {
        const Tags tg = find_tags(ch, d);
        const int first = d.l_seq > 0 ? shifted(qual[0], opt.illumina ? 1 : 0) : 0;
        n.plan = plan_record(d.pos, d.l_seq, d.flag, cig, d.n_cigar, first, tg.bq != nullptr, tg.zq, opt.redo, ref_len);
        if (n.plan.hmm && n.plan.xe > n.plan.xb) {
            lo = std::min<int64_t>(lo, n.plan.xb);
            hi = std::max<int64_t>(hi, n.plan.xe);
        }
    }
    n.lo = lo;
    n.hi = hi;
    return n;
}

}  // namespace

int reference_quality(double z) { return (int)(-4.343 * std::log(z) + .499); }

const Tables& tables()
{
    static Tables t;
    static std::once_flag once;
    std::call_once(once, [] {
        for (int i = 0; i < 256; ++i) t.qual2prob[i] = (float)std::pow(10, -i / 10.);
        for (int j = 0; j < 101; ++j) {
            // the doubles in (0, 1] ordered as their bit patterns: lo has a quality >= j + 1, hi has not
            uint64_t lo = 1, hi;
            const double one = 1.;
            std::memcpy(&hi, &one, 8);
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                double z;
                std::memcpy(&z, &mid, 8);
                if (reference_quality(z) >= j + 1) lo = mid;
                else hi = mid;
            }
            std::memcpy(&t.thresh[j], &lo, 8);
        }
    });
    return t;
}

Options options_of(int incl_flags, int adjust_mq)
{
    Options o;
    o.illumina = (incl_flags & 128) != 0;
    o.realn = (incl_flags & 16) != 0;
    o.redo = (incl_flags & 64) != 0;
    o.cap = adjust_mq;
    return o;
}

Tags find_tags(const bamio::Chunk& ch, const bamio::RecordDesc& d)
{
    Tags t;
    const std::vector<uint8_t>& b = ch.bytes;
    if (d.data < 36 || (size_t)d.data > b.size()) return t;
    const uint64_t o = (uint64_t)d.data - 36;
    const uint64_t block = le32(b.data() + o);
    const uint64_t end = o + 4 + block;
    const uint64_t var = (uint64_t)d.l_read_name + 4ull * d.n_cigar + ((uint64_t)d.l_seq + 1) / 2 + (uint64_t)d.l_seq;
    uint64_t p = (uint64_t)d.data + var;
    if (end > b.size() || p > end) return t;
    bool have_bq = false, have_zq = false;
    auto width = [](uint8_t ty) -> uint64_t {
        switch (ty) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
        }
    };
    while (end - p >= 3) {
        const uint8_t t0 = b[p], t1 = b[p + 1], ty = b[p + 2];
        p += 3;
        uint64_t len = 0;
        if (ty == 'Z' || ty == 'H') {
            const void* nul = end > p ? std::memchr(b.data() + p, 0, (size_t)(end - p)) : nullptr;
            if (!nul) return t;
            len = (uint64_t)((const uint8_t*)nul - (b.data() + p)) + 1;
            if (ty == 'Z' && t1 == 'Q') {
                if (t0 == 'B' && !have_bq) {
                    have_bq = true;
                    if (len - 1 >= (uint64_t)d.l_seq) t.bq = b.data() + p;
                } else if (t0 == 'Z' && !have_zq) {
                    have_zq = true;
                    t.zq = true;
                }
            }
        } else if (ty == 'B') {
            if (end - p < 5) return t;
            const uint64_t w = width(b[p]);
            const uint64_t count = le32(b.data() + p + 1);
            if (w == 0 || count > (end - p - 5) / w) return t;
            len = 5 + count * w;
        } else {
            len = width(ty);
            if (len == 0 || len > end - p) return t;
        }
        p += len;
    }
    return t;
}

int load_spans(const bamio::Scan& scan, const std::string& fasta_path, const Options& opt, Spans* out, std::string* err)
{
    const double t0 = now_s();
    out->codes.clear();
    out->of_chunk.assign(scan.chunks.size(), {});
    out->span_of_rec.assign(scan.chunks.size(), {});
    out->ref_len.assign(scan.ref_name.size(), -1);
    out->bytes_read = 0;
    out->seconds = 0;
    if (!opt.needs_fasta()) return fasta::kOk;
    fasta::Index idx;
    if (int rc = fasta::open_index(fasta_path, &idx, err)) return rc;
    std::vector<int> seq_of_tid(scan.ref_name.size(), -1);
    for (size_t t = 0; t < scan.ref_name.size(); ++t) {
        const int s = idx.find(scan.ref_name[t]);
        seq_of_tid[t] = s;
        if (s >= 0) out->ref_len[t] = std::min<int64_t>(idx.seqs[(size_t)s].length, 0x7fffffff);
    }
    uint64_t total = 0;
    for (size_t ci = 0; ci < scan.chunks.size(); ++ci) {
        const bamio::Chunk& ch = scan.chunks[ci];
        if (ch.tid < 0 || (size_t)ch.tid >= out->ref_len.size()) continue;
        const int64_t ref_len = out->ref_len[(size_t)ch.tid];
        if (ref_len < 0) continue;
        std::vector<Spans::Span>& sp = out->of_chunk[ci];
        std::vector<uint32_t>& of_rec = out->span_of_rec[ci];
        of_rec.assign(ch.recs.size(), 0);
        for (size_t ri = 0; ri < ch.recs.size(); ++ri) {
            const Need n = need_of(ch, ch.recs[ri], opt, ref_len);
            if (n.lo >= n.hi) {
                of_rec[ri] = sp.empty() ? 0u : (uint32_t)(sp.size() - 1);
                continue;
            }
            if (sp.empty() || n.lo > sp.back().end + kSpanGap) {
                Spans::Span one;
                one.beg = n.lo;
                one.end = n.hi;
                sp.push_back(one);
            } else {
                sp.back().beg = std::min(sp.back().beg, n.lo);
                sp.back().end = std::max(sp.back().end, n.hi);
            }
            of_rec[ri] = (uint32_t)(sp.size() - 1);
        }
        for (Spans::Span& one : sp) {
            one.off = total;
            total += (uint64_t)(one.end - one.beg);
        }
        if (total > 0xfff00000ull) {
            *err = "--ApplyBAQ: the records touch more than 4 GiB of the reference";
            return fasta::kErrInvalid;
        }
    }
    out->codes.resize((size_t)total);
    fasta::Reader reader(idx);
    for (size_t ci = 0; ci < scan.chunks.size(); ++ci)
        for (const Spans::Span& one : out->of_chunk[ci]) {
            if (int rc = reader.fetch_nt16(seq_of_tid[(size_t)scan.chunks[ci].tid], one.beg, one.end, out->codes.data() + one.off, err))
                return rc;
            out->bytes_read += one.end - one.beg;
        }
    out->seconds = now_s() - t0;
    return fasta::kOk;
}

Task make_task(const bamio::Scan& scan, size_t ci, size_t ri, const Spans& spans, const Options& opt, const uint8_t** bq)
{
    const bamio::Chunk& ch = scan.chunks[ci];
    const bamio::RecordDesc& d = ch.recs[ri];
    Task t;
    std::memset(&t, 0, sizeof(t));
    t.bw = 7;
    t.bq_off = 0xffffffffu;
    *bq = nullptr;
    const int64_t ref_len = d.tid >= 0 && (size_t)d.tid < spans.ref_len.size() ? spans.ref_len[(size_t)d.tid] : -1;
    if (ref_len < 0) {
        t.outcome = opt.needs_fasta() ? kNoReference : kNotAsked;
        return t;
    }
    t.ref_len = (int32_t)ref_len;
    if (d.pos >= ref_len) {
        t.outcome = kOutside;
        return t;
    }
    static const Spans::Span kNone;
    const Spans::Span& sp = ri < spans.span_of_rec[ci].size() && spans.span_of_rec[ci][ri] < spans.of_chunk[ci].size()
                                ? spans.of_chunk[ci][spans.span_of_rec[ci][ri]] : kNone;
    t.span_beg = (int32_t)sp.beg;
    t.span_off = (uint32_t)sp.off;
    const Need n = need_of(ch, d, opt, ref_len);
    t.outcome = n.plan.outcome;
    if (opt.realn) {
        if (n.plan.hmm) {
            t.kind = 2;
            t.xb = n.plan.xb;
            t.l_ref = n.plan.xe - n.plan.xb;
            t.bw = n.plan.bw;
        } else if (n.plan.outcome == kTagApplied) {
            t.kind = 1;
            *bq = find_tags(ch, d).bq;
        }
    }
    t.cap = opt.cap_on() ? 1 : 0;
    // (load_spans sized the chunk's span by the same need_of: the window and the walk lie inside it)
    if (n.lo < n.hi && (n.lo < sp.beg || n.hi > sp.end)) {
        t.kind = 0;
        t.cap = 0;
        t.outcome = kNoReference;
    }
    return t;
}

int cap_finish(const int32_t cap4[4], int thres)
{
    const int mm = cap4[0], q = cap4[1], len = cap4[2], clip_q = cap4[3];
    double t = 1;
    for (int i = 0; i < mm; ++i) t *= (double)len / (i + 1);
    t = q - 4.343 * std::log(t) + clip_q / 5.;
    if (t > thres) return -1;
    if (t < 0) t = 0;
    t = std::sqrt((thres - t) / thres) * thres;
    return (int)(t + .499);
}

Finished finish_record(int mapq, const Task& t, const int32_t cap4[4], const Options& opt, vb2_baq_stats* st)
{
    Finished f{mapq, t.outcome};
    if (f.outcome == kOutside) {
        f.mapq = -1;
    } else if (t.cap) {
        f.mapq = capped_mapq(mapq, cap_finish(cap4, opt.cap));
        if (f.mapq < 0) f.outcome = kCapDropped;
    }
    ++st->records;
    switch (f.outcome) {
    case kRealigned: ++st->realigned; break;
    case kAlone: ++st->left_alone; break;
    case kTagApplied: ++st->tag_applied; break;
    case kNoReference: ++st->no_reference; break;
    case kOutside: ++st->dropped_outside; break;
    case kCapDropped: ++st->dropped_cap; break;
    default: ++st->not_asked; break;
    }
    return f;
}

int run_record(const bamio::RecordDesc& d, const uint8_t* rec, const Task& t, const uint8_t* span_codes, const uint8_t* extra,
               const Options& opt, uint8_t* out_qual, int32_t cap4[4], std::vector<double>* scratch)
{
    const uint8_t* cig = rec + d.l_read_name;
    const uint8_t* seq = cig + 4ull * d.n_cigar;
    const uint8_t* qual = seq + ((uint64_t)d.l_seq + 1) / 2;
    const int ill = opt.illumina ? 1 : 0;
    int undefined = 0;
    copy_quals(qual, d.l_seq, ill, out_qual, 0, 1);
    if (t.kind == 1) {
        apply_bq_tag(extra + t.bq_off, d.l_seq, out_qual, 0, 1);
    } else if (t.kind == 2) {
        scratch->assign((size_t)(work_bytes(t.l_ref, d.l_seq, t.bw) / 8) + 1, 0.);
        const Work w = carve(scratch->data(), t.l_ref, d.l_seq, t.bw);
        const Ref ref{span_codes + t.span_off + (t.xb - t.span_beg), 1};
        const Query qy{nullptr, seq, qual, ill};
        undefined = glocal(ref, t.l_ref, qy, d.l_seq, t.bw, &tables(), w, 0, 1, d.l_seq, NoSync());
        extend_apply(d.pos, d.l_seq, cig, d.n_cigar, t.xb, w, out_qual);
    }
    cap4[0] = cap4[1] = cap4[2] = cap4[3] = 0;
    if (t.cap) cap_walk(d.pos, cig, d.n_cigar, seq, out_qual, d.l_seq, span_codes + t.span_off, t.span_beg, t.ref_len, cap4);
    return undefined;
}

int run_case(const uint8_t* ref, int l_ref, const uint8_t* query, const uint8_t* qual, int l_query, int conf_bw, int32_t* state,
             uint8_t* q)
{
    if (l_query <= 0) return 0;
    std::vector<double> scratch((size_t)(work_bytes(l_ref, l_query, conf_bw) / 8) + 1, 0.);
    const Work w = carve(scratch.data(), l_ref, l_query, conf_bw);
    const Ref r{ref, 0};
    const Query qy{query, nullptr, qual, 0};
    const int undefined = glocal(r, l_ref, qy, l_query, conf_bw, &tables(), w, 0, 1, l_query, NoSync());
    for (int i = 0; i < l_query; ++i) {
        state[i] = w.state[i];
        q[i] = w.q[i];
    }
    return undefined;
}

}  // namespace baq
}  // namespace vb2
