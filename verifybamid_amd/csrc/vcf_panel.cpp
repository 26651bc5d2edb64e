// vcf_panel.cpp -- the reference-panel VCF reader of --RefVCF: SVDcalculator::ReadVcf (SVDcalculator.cpp:22-228)
// with the parts of libVcf it depends on (libVcfFile.cpp: iterateMarker :473-530, setFilters :573, setAlts,
// setSample :909-940), rule for rule.  Host only: no HIP call.
//
// Structure: one thread inflates (zlib: plain, gzip or BGZF) into blocks of whole lines; a pool of parser threads
// turns each block into per-line outcomes and the kept lines' genotypes; the calling thread merges the blocks in file
// order (the duplicate check depends on the previous KEPT marker, so it is the one sequential rule) and hands the
// genotypes to the sink block by block.
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <map>
#include <mutex>
#include <sstream>
#include <thread>

#include "context.h"
#include "panel.h"

namespace vb2 {

namespace {

constexpr int kMaxPhred = 255;
constexpr size_t kBlockBytes = 4u << 20;

struct Str {
    const char* p;
    size_t n;
    bool eq(const char* s) const { return std::strlen(s) == n && std::memcmp(p, s, n) == 0; }
    std::string str() const { return std::string(p, n); }
};

// String::AsInteger (statgen/StringBasics.cpp:1015-1066): optional '-', optional 0x, digits up to the first other
// character; the partial value counts
long as_integer(Str s)
{
    size_t pos = 0;
    long sign = 1, base = 10, v = 0;
    if (pos == s.n) return 0;
    if (s.p[pos] == '-') sign = -1, ++pos;
    if (s.n > pos + 2 && s.p[pos] == '0' && (s.p[pos + 1] == 'x' || s.p[pos + 1] == 'X')) base = 16, pos += 2;
    for (; pos < s.n; ++pos) {
        const char d = (char)std::toupper((unsigned char)s.p[pos]);
        if (d >= '0' && d <= '9') v = v * base + (d - '0');
        else if (d >= 'A' && d <= 'F' && base == 16) v = v * base + (d - 'A' + 10);
        else break;
    }
    return sign * v;
}

double as_double(Str s)
{
    char buf[64];
    const size_t n = std::min(s.n, sizeof(buf) - 1);
    std::memcpy(buf, s.p, n);
    buf[n] = 0;
    return std::atof(buf);
}

// StringArray::AddColumns: every separator splits, empty fields kept; an empty string has no column
int split_columns(Str s, char ch, Str* out, int max_out)
{
    if (s.n == 0) return 0;
    int k = 0;
    size_t b = 0;
    for (size_t i = 0; i <= s.n; ++i) {
        if (i == s.n || s.p[i] == ch) {
            if (k < max_out) out[k] = Str{s.p + b, i - b};
            ++k;
            b = i + 1;
        }
    }
    return k;
}

// StringArray::AddTokens: runs of separators split, empty tokens dropped
int split_tokens(Str s, const char* seps, Str* out, int max_out)
{
    int k = 0;
    size_t i = 0;
    while (i < s.n) {
        while (i < s.n && std::strchr(seps, s.p[i])) ++i;
        const size_t b = i;
        while (i < s.n && !std::strchr(seps, s.p[i])) ++i;
        if (b < s.n) {
            if (k < max_out) out[k] = Str{s.p + b, i - b};
            ++k;
        }
    }
    return k;
}

enum Kind : uint8_t { kKept, kSkipFilter, kSkipMulti, kSkipNonSnp, kSkipChr, kSkipMissing, kFatalPre, kFatalPost, kEnd };

struct LineOut {
    Kind kind;
    char ref, alt;
    int32_t pos;
    float miss_rate;
    Str chr;                 // points into the block's text
    std::string msg;         // fatal text / the filter token
};

struct Block {
    std::string text;
    int64_t first_line = 0;  // 1-based file line number of the block's first line
};

struct Parsed {
    std::vector<LineOut> lines;
    std::vector<int8_t> geno;   // kept lines x N
};

struct ParseCtx {
    int32_t n;                              // header sample count
    const std::unordered_set<std::string>* include;
};

void parse_block(const Block& b, const ParseCtx& pc, Parsed* out)
{
    const int32_t N = pc.n;
    const char* p = b.text.data();
    const char* end = p + b.text.size();
    std::vector<Str> cols;
    cols.reserve((size_t)N + 16);
    std::vector<Str> sub(64);
    int64_t lineno = b.first_line;
    for (; p < end; ++lineno) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(end - p));
        if (!nl) nl = end;
        Str line{p, (size_t)(nl - p)};
        p = nl + 1;
        if (line.n && line.p[line.n - 1] == '\r') --line.n;
        LineOut lo{};
        lo.kind = kKept;
        if (line.n == 0) {           // String::ReadLine returns 0 on an empty line: iterateMarker ends the file there
            lo.kind = kEnd;
            out->lines.push_back(std::move(lo));
            return;
        }
        cols.clear();
        {
            size_t bpos = 0;
            for (size_t i = 0; i <= line.n; ++i)
                if (i == line.n || line.p[i] == '\t') {
                    cols.push_back(Str{line.p + bpos, i - bpos});
                    bpos = i + 1;
                }
        }
        auto fatal_pre = [&](const std::string& m) {
            lo.kind = kFatalPre;
            lo.msg = m + " See line " + std::to_string(lineno) + ".";
        };
        if (cols.size() < 9) {
            fatal_pre("Cannot recognize GT, GL or PL key in FORMAT field (a line with fewer than 9 columns).");
            out->lines.push_back(std::move(lo));
            continue;
        }
        lo.chr = cols[0];
        lo.pos = (int32_t)as_integer(cols[1]);
        const size_t offset = cols.size() > 9 && cols[9].n == 0 ? 10 : 9;   // iterateMarker :514 (glfMultiples)
        Str keys[64];
        const int nkey = split_columns(cols[8], ':', keys, 64);
        if ((int64_t)(cols.size() - offset) != N) {
            fatal_pre("The number of sample columns (" + std::to_string(cols.size() - offset) +
                      ") differs from the header's (" + std::to_string(N) + ").");
            out->lines.push_back(std::move(lo));
            continue;
        }
        // libVcfFile.cpp:931-934: a value's field count must equal FORMAT's ('.' and './.' are missing)
        bool bad = false;
        for (int32_t i = 0; i < N && !bad; ++i) {
            const Str s = cols[offset + i];
            if (s.eq(".") || s.eq("./.")) continue;
            int k = s.n ? 1 : 0;
            for (size_t j = 0; j < s.n; ++j) k += s.p[j] == ':';
            if (k != nkey) {
                char m[256];
                std::snprintf(m, sizeof(m), "# values = %.*s do not match with # fields in FORMAT field = %d at sampleIndex = %d",
                              (int)std::min<size_t>(s.n, 100), s.p, nkey, (int)i);
                fatal_pre(m);
                bad = true;
            }
        }
        if (bad) {
            out->lines.push_back(std::move(lo));
            continue;
        }
        Str filt[2];
        const int nf = split_columns(cols[6], ';', filt, 2);
        if (nf != 1 || !filt[0].eq("PASS")) {
            lo.kind = kSkipFilter;
            lo.msg = nf ? filt[0].str() : std::string();
            out->lines.push_back(std::move(lo));
            continue;
        }
        const Str altcol = cols[4];
        int nalt = 1;
        for (size_t j = 0; j < altcol.n; ++j) nalt += altcol.p[j] == ',';
        if (nalt > 1) {
            lo.kind = kSkipMulti;
            out->lines.push_back(std::move(lo));
            continue;
        }
        if (cols[3].n > 1 || altcol.n > 1) {
            lo.kind = kSkipNonSnp;
            out->lines.push_back(std::move(lo));
            continue;
        }
        if (!pc.include->empty() && !pc.include->count(lo.chr.str())) {
            lo.kind = kSkipChr;
            out->lines.push_back(std::move(lo));
            continue;
        }
        lo.ref = (char)std::toupper((unsigned char)(cols[3].n ? cols[3].p[0] : 0));
        lo.alt = (char)std::toupper((unsigned char)(altcol.n ? altcol.p[0] : 0));
        int idxPL = -1, idxGL = -1, idxGT = -1;
        for (int k = nkey - 1; k >= 0; --k) {     // StringArray::Find: the first match
            if (keys[k].eq("PL")) idxPL = k;
            if (keys[k].eq("GL")) idxGL = k;
            if (keys[k].eq("GT")) idxGT = k;
        }
        if (idxPL < 0 && idxGL < 0 && idxGT < 0) {
            lo.kind = kFatalPost;
            lo.msg = "Cannot recognize GT, GL or PL key in FORMAT field";
            out->lines.push_back(std::move(lo));
            continue;
        }
        const size_t g0 = out->geno.size();
        out->geno.resize(g0 + (size_t)N, (int8_t)-1);
        int8_t* g = out->geno.data() + g0;
        int nmiss = 0;
        Str f[64];
        for (int32_t i = 0; i < N; ++i) {
            const Str s = cols[offset + i];
            if (s.eq(".") || s.eq("./.")) {
                ++nmiss;
                continue;
            }
            split_columns(s, ':', f, 64);
            long ph[3] = {0, 0, 0};
            bool parsed = false;
            if (idxPL >= 0) {
                if (split_tokens(f[idxPL], ",", sub.data(), 4) == 3 && !sub[0].eq(".") && !sub[1].eq(".") && !sub[2].eq(".")) {
                    for (int t = 0; t < 3; ++t) ph[t] = as_integer(sub[t]);
                    parsed = true;
                }
            }
            if (!parsed && idxGL >= 0) {
                if (split_tokens(f[idxGL], ",", sub.data(), 4) == 3 && !sub[0].eq(".") && !sub[1].eq(".") && !sub[2].eq(".")) {
                    for (int t = 0; t < 3; ++t) {
                        const double d = -10. * as_double(sub[t]);
                        ph[t] = d >= 2147483647. ? INT_MAX : d <= -2147483648. ? INT_MIN : static_cast<int>(d);
                    }
                    parsed = true;
                }
            }
            if (!parsed && idxGT >= 0) {
                if (split_tokens(f[idxGT], "|/", sub.data(), 3) == 2 && !sub[0].eq(".") && !sub[1].eq(".")) {
                    const long gsum = as_integer(sub[0]) + as_integer(sub[1]);
                    if (gsum == 0) ph[0] = 0, ph[1] = 30, ph[2] = 50;
                    else if (gsum == 1) ph[0] = 50, ph[1] = 0, ph[2] = 50;
                    else ph[0] = 50, ph[1] = 30, ph[2] = 0;
                    parsed = true;
                }
            }
            if (!parsed) {
                ++nmiss;
                continue;
            }
            if (ph[0] < 0 || ph[1] < 0 || ph[2] < 0) {
                lo.kind = kFatalPost;
                lo.msg = "Negative PL or Positive GL observed";
                break;
            }
            int mg = -1;
            long mp = kMaxPhred;
            for (int t = 0; t < 3; ++t) {
                const long v = std::min<long>(ph[t], kMaxPhred);
                if (v < mp) mp = v, mg = t;
            }
            g[i] = (int8_t)mg;
        }
        if (lo.kind == kKept) {
            lo.miss_rate = static_cast<float>(nmiss) / N;
            if (lo.miss_rate > 0.2f) lo.kind = kSkipMissing;
        }
        if (lo.kind != kKept) out->geno.resize(g0);
        out->lines.push_back(std::move(lo));
    }
}

// The inflating thread: whole-line blocks into a bounded queue
class Inflater {
public:
    explicit Inflater(gzFile f, size_t max_queued) : f_(f), max_(max_queued) { th_ = std::thread([this] { run(); }); }
    ~Inflater()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
    }
    // false = end of input (or error: see error())
    bool next(std::string* out)
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !q_.empty() || done_; });
        if (q_.empty()) return false;
        *out = std::move(q_.front());
        q_.pop_front();
        cv_.notify_all();
        return true;
    }
    const std::string& error() const { return err_; }

private:
    void run()
    {
        std::string carry;
        std::vector<char> buf(kBlockBytes);
        for (;;) {
            const int n = gzread(f_, buf.data(), (unsigned)buf.size());
            if (n < 0) {
                int e = 0;
                const char* m = gzerror(f_, &e);
                std::lock_guard<std::mutex> lk(m_);
                err_ = std::string("inflating the VCF failed: ") + (m ? m : "?");
                break;
            }
            std::string blk;
            if (n == 0) {
                if (carry.empty()) break;
                blk.swap(carry);
            } else {
                const char* nl = nullptr;
                for (int i = n - 1; i >= 0; --i)
                    if (buf[i] == '\n') { nl = buf.data() + i; break; }
                if (!nl) {
                    carry.append(buf.data(), (size_t)n);
                    continue;
                }
                blk.reserve(carry.size() + (size_t)(nl - buf.data()) + 1);
                blk.swap(carry);
                blk.append(buf.data(), (size_t)(nl - buf.data()) + 1);
                carry.assign(nl + 1, (size_t)(buf.data() + n - (nl + 1)));
            }
            std::unique_lock<std::mutex> lk(m_);
            cv_.wait(lk, [&] { return q_.size() < max_ || stop_; });
            if (stop_) return;
            q_.push_back(std::move(blk));
            cv_.notify_all();
            if (n == 0) break;
        }
        std::lock_guard<std::mutex> lk(m_);
        done_ = true;
        cv_.notify_all();
    }

    gzFile f_;
    size_t max_;
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<std::string> q_;
    bool done_ = false, stop_ = false;
    std::string err_;
};

struct GzCloser {
    gzFile f;
    ~GzCloser() { if (f) gzclose(f); }
};

void warn(bool on, const std::string& m)
{
    if (on) std::fprintf(stderr, "WARNING - %s\n", m.c_str());
}

}  // namespace

std::unordered_set<std::string> parse_include_chr(const char* list)
{
    static const char* kDefault =
        "1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,"
        "chr1,chr2,chr3,chr4,chr5,chr6,chr7,chr8,chr9,chr10,"
        "chr11,chr12,chr13,chr14,chr15,chr16,chr17,chr18,chr19,"
        "chr20,chr21,chr22";
    std::unordered_set<std::string> out;
    std::stringstream ss(list ? list : kDefault);
    std::string tok;
    while (std::getline(ss, tok, ','))
        if (!tok.empty()) out.insert(tok);
    return out;
}

int read_vcf(const std::string& path, const std::unordered_set<std::string>& includeChr, int num_thread,
             bool notices, VcfMarkers* mk, const HeaderSink& on_header, const GenotypeSink& sink)
{
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) {
        set_error("Cannot open file " + path);
        return VB2_ERR_IO;
    }
    GzCloser closer{f};
    gzbuffer(f, 1 << 20);
    const int nth = std::max(1, std::min(num_thread > 0 ? num_thread : 4, 64));
    Inflater inf(f, (size_t)(2 * nth + 2));

    // header: ## lines, then #CHROM ... FORMAT samples
    std::string blk;
    size_t at = 0;
    int64_t lineno = 0;
    bool have_header = false;
    while (!have_header) {
        if (at >= blk.size()) {
            if (!inf.next(&blk)) break;
            at = 0;
        }
        const size_t nl = blk.find('\n', at);
        std::string line = blk.substr(at, nl == std::string::npos ? std::string::npos : nl - at);
        at = nl == std::string::npos ? blk.size() : nl + 1;
        ++lineno;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.compare(0, 2, "##") == 0) continue;
        if (line.compare(0, 6, "#CHROM") != 0) {
            set_error("The VCF file " + path + " has no #CHROM header line before its first record");
            return VB2_ERR_INVALID;
        }
        std::vector<std::string> h;
        std::stringstream ss(line);
        std::string tok;
        while (std::getline(ss, tok, '\t')) h.push_back(tok);
        for (size_t i = 9; i < h.size(); ++i) mk->samples.push_back(h[i]);
        have_header = true;
    }
    if (!inf.error().empty()) {
        set_error(inf.error());
        return VB2_ERR_IO;
    }
    if (!have_header) {
        set_error("The VCF file " + path + " has no #CHROM header line");
        return VB2_ERR_INVALID;
    }
    const int32_t N = (int32_t)mk->samples.size();
    if (N == 0) {
        set_error("No individual genotype information exist in the input VCF file " + path);
        return VB2_ERR_INVALID;
    }
    mk->num_sample = N;
    if (!includeChr.empty() && notices)
        std::fprintf(stderr, "NOTICE - Filtering to %d chromosome(s) specified by --IncludeChr\n", (int)includeChr.size());
    if (on_header) on_header(N);

    ParseCtx pc{N, &includeChr};
    std::deque<std::pair<std::shared_ptr<Block>, std::future<Parsed>>> inflight;
    auto submit = [&](std::string&& text) {
        auto b = std::make_shared<Block>();
        b->text = std::move(text);
        b->first_line = lineno + 1;
        lineno += (int64_t)std::count(b->text.begin(), b->text.end(), '\n');
        if (!b->text.empty() && b->text.back() != '\n') ++lineno;
        inflight.emplace_back(b, std::async(std::launch::async, [b, pc] {
                                  Parsed r;
                                  parse_block(*b, pc, &r);
                                  return r;
                              }));
    };
    if (at < blk.size()) submit(blk.substr(at));

    std::string prev_name;
    std::map<std::string, int32_t> chr_idx;
    bool ended = false;
    int rc = VB2_OK;
    auto merge = [&](Block& b, Parsed& r) {
        size_t gi = 0;
        std::vector<std::pair<int64_t, int64_t>> runs;
        for (const LineOut& lo : r.lines) {
            if (lo.kind == kEnd) {
                ended = true;
                break;
            }
            if (lo.kind == kFatalPre) {
                set_error(lo.msg);
                return (int)VB2_ERR_INVALID;
            }
            const std::string name = lo.chr.str() + ":" + std::to_string(lo.pos);
            if (name == prev_name) {
                set_error("Duplicated Marker: " + name);
                return (int)VB2_ERR_INVALID;
            }
            switch (lo.kind) {
            case kSkipFilter: warn(notices, "Skip filtered (" + lo.msg + ") marker: " + name); continue;
            case kSkipMulti: warn(notices, "Skip non-Biallelic marker: " + name); continue;
            case kSkipNonSnp: warn(notices, "Skip non-SNP marker: " + name); continue;
            case kSkipChr: continue;
            case kFatalPost: set_error(lo.msg); return (int)VB2_ERR_INVALID;
            case kSkipMissing: {
                char m[64];
                std::snprintf(m, sizeof(m), "%f", lo.miss_rate);
                warn(notices, "Skip marker (" + name + ") with high missing rate (" + m + " > 0.2) in genotype fields.");
                continue;
            }
            default: break;
            }
            const std::string chr = lo.chr.str();
            auto it = chr_idx.find(chr);
            if (it == chr_idx.end()) {
                it = chr_idx.emplace(chr, (int32_t)mk->chr_names.size()).first;
                mk->chr_names.push_back(chr);
            }
            mk->chr_index.push_back(it->second);
            mk->pos.push_back(lo.pos);
            mk->ref.push_back(lo.ref);
            mk->alt.push_back(lo.alt);
            ++gi;
            prev_name = name;
        }
        const int64_t first = mk->num_marker;
        mk->num_marker += (int64_t)gi;
        (void)b;
        return gi && sink ? sink(r.geno.data(), first, (int64_t)gi) : (int)VB2_OK;
    };
    try {
        for (;;) {
            while (!ended && (int)inflight.size() < 2 * nth) {
                std::string t;
                if (!inf.next(&t)) break;
                submit(std::move(t));
            }
            if (inflight.empty()) break;
            auto front = std::move(inflight.front());
            inflight.pop_front();
            Parsed r = front.second.get();
            if (ended) continue;
            rc = merge(*front.first, r);
            if (rc != VB2_OK) break;
        }
    } catch (const std::exception& e) {
        set_error(std::string("reading the VCF: ") + e.what());
        rc = VB2_ERR_INVALID;
    }
    for (auto& x : inflight) x.second.wait();
    if (rc != VB2_OK) return rc;
    if (!inf.error().empty()) {
        set_error(inf.error());
        return VB2_ERR_IO;
    }
    if (notices) {
        std::map<std::string, int64_t> counts;
        for (int32_t c : mk->chr_index) counts[mk->chr_names[c]]++;
        std::fprintf(stderr, "NOTICE - Markers retained across %d chromosome(s):\n", (int)counts.size());
        for (const auto& kv : counts) std::fprintf(stderr, "NOTICE -   %s: %lld markers\n", kv.first.c_str(), (long long)kv.second);
    }
    return VB2_OK;
}

}  // namespace vb2
