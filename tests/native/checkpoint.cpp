// What a checkpoint blob's entries mean (flink_amd/csrc/gw_checkpoint.h) on its own, without a
// GPU: reads a file of cases -- int64 kind, int64 n, n int64 parameters, int64 length, the
// blob's bytes -- prints one line per case and writes the blobs it built, length-prefixed, to
// a second file.  Every input blob sits in a heap block of exactly its length, so the
// sanitizers see any read outside it.  tests/test_checkpoint_host.py.
//   kind 0, a valid blob of the operator in the parameters (Spec's fields, then J): decode,
//     encode as a restore leaves the state (nothing fired, no pane cells), decode again (the
//     same entries), encode again (the same bytes); the blob goes out.  J > 0: the input cut
//     into J window classes and merged again goes out too.  "ok <entries>"
//   kind 1, the same blob kind: prints the decoded windows and key hashes.
//   kind 2, a damaged blob (parameters: Spec, a key group): the operator's own decoder as a
//     restore runs it, with the round trip of kind 0 when it accepts; then every decoder, cut
//     and blob tool on the raw bytes.  "dec=<0|1> slice=<code> keys=<invalid | k,k,...> why=<the decoder's reason>"
//   kind 3, no blob (parameters: key A, key B, fired_k, state_lo, lateness): the hand-made
//     pane case of encode_windows; the blob goes out.
//   kind 4, no blob: a hand-made first-element blob split into the two operators' blobs and
//     joined again.  "ok"
// A failed check prints "FAIL ..." and the program ends with status 1.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "gw_checkpoint.h"

namespace snap = gw::snap;
namespace ckpt = gw::ckpt;
using ckpt::i128;
typedef std::vector<uint8_t> Bytes;

static FILE* g_out;
static void emit(const Bytes& b) {
    const int64_t n = (int64_t)b.size();
    fwrite(&n, 8, 1, g_out);
    if (n) fwrite(b.data(), (size_t)n, 1, g_out);
}
[[noreturn]] static void fail(const char* what) {
    printf("FAIL %s\n", what);
    exit(1);
}
static const i128 kBelow = -((i128)1 << 100);  // below every window index

static ckpt::Spec spec_of(const int64_t* p) {
    ckpt::Spec s{};
    s.agg = (int32_t)p[0]; s.assigner = (int32_t)p[1]; s.trigger = (int32_t)p[2]; s.max_parallelism = (int32_t)p[3];
    s.size = p[4]; s.slide = p[5]; s.cfg_slide = p[6]; s.offset = p[7]; s.gap = p[8]; s.allowed_lateness = p[9];
    s.n = p[10]; s.m = p[11]; s.ew = p[12];
    return s;
}
constexpr int kSpecParams = 13;

// A blob's entries for its operator, in one order.
struct Decoded {
    snap::Header hd;
    std::vector<std::array<int64_t, 5>> win;  // (key, k, a0, a1, flags)
    std::vector<std::vector<int64_t>> ent;    // s.ew words each
    std::vector<std::pair<int64_t, int32_t>> hashes;
    bool same(const Decoded& o) const { return win == o.win && ent == o.ent && hashes == o.hashes; }
};

// As gw_restore reads a blob: header, the operator's kind, payload, decoder, key hashes.
// g_why: why the last blob was rejected.
static std::string g_why;
static bool decode(const ckpt::Spec& s, const uint8_t* b, int64_t len, Decoded& d) {
    snap::Cursor c;
    snap::Err e = snap::header(b, len, 1, snap::kMaxVersion, d.hd);
    if (!e && !s.matches(d.hd)) e = snap::invalid(ckpt::kOtherOperator);
    if (!e) e = snap::payload(b, len, d.hd, c);
    ckpt::HashPairs hp;
    std::vector<int64_t> ent;
    std::vector<ckpt::WindowEntry> win;
    std::string why;
    if (!e)
        e = s.ew == 0                         ? ckpt::decode_windows(s, d.hd, c, win, hp, why)
            : s.session()                     ? ckpt::decode_sessions(s, d.hd, c, ent, hp)
            : s.assigner == GW_COUNT_TUMBLING ? ckpt::decode_count(s, d.hd, c, ent, hp)
                                              : ckpt::decode_slots(s, d.hd, c, ent, hp);
    if (!e) e = hp.check();
    g_why = e.reason;
    if (e) return false;
    for (const auto& x : win) d.win.push_back({x.key, x.k, x.a0, x.a1, (int64_t)x.flags});
    const int64_t ew = s.session() ? 6 : s.ew;
    for (size_t i = 0; ew && i + ew <= ent.size(); i += ew) d.ent.emplace_back(ent.begin() + i, ent.begin() + i + ew);
    for (size_t i = 0; i < hp.keys.size(); ++i) d.hashes.push_back({hp.keys[i], hp.hashes[i]});
    std::sort(d.win.begin(), d.win.end());
    std::sort(d.ent.begin(), d.ent.end());
    std::sort(d.hashes.begin(), d.hashes.end());
    d.hashes.erase(std::unique(d.hashes.begin(), d.hashes.end()), d.hashes.end());
    return true;
}

// The blob of the state a restore of d leaves: nothing fired, no pane cells.
static Bytes encode(const ckpt::Spec& s, const Decoded& d) {
    ckpt::KeyHashes kh;
    for (const auto& p : d.hashes) {
        if (p.first == gw::kEmptyKey) { kh.has_min = true; kh.min_hash = p.second; }
        else kh.kv.push_back(p);
    }
    const int32_t lo = d.hd.kg_lo, hi = d.hd.kg_hi;
    snap::Writer w;
    snap::Header hd;
    if (s.ew == 0) {
        std::vector<ckpt::WindowEntry> ov;
        for (const auto& e : d.win) ov.push_back({e[0], e[1], e[2], e[3], (uint32_t)e[4]});
        const std::vector<int64_t> col[4];
        if (ckpt::encode_windows(s, kh, lo, hi, col, {}, ov, kBelow, kBelow, w, hd)) fail("encode_windows");
    } else {
        std::vector<int64_t> ent;
        std::vector<int32_t> kgs;
        for (const auto& e : d.ent) {
            ent.insert(ent.end(), e.begin(), e.end());
            kgs.push_back(kh.key_group(e[0], s.max_parallelism));
        }
        hd = s.session()                        ? ckpt::encode_sessions(s, kh, lo, hi, ent, kgs, w)
             : s.assigner == GW_COUNT_TUMBLING ? ckpt::encode_count(s, kh, lo, hi, ent, kgs, w)
                                               : ckpt::encode_slots(s, kh, lo, hi, ent, kgs, w);
    }
    return w.finish(hd);
}

// decode, encode, decode (the same entries), encode (the same bytes); -> the first encoding
static Bytes round_trip(const ckpt::Spec& s, const Decoded& d1) {
    const Bytes e1 = encode(s, d1);
    Decoded d2;
    if (!decode(s, e1.data(), (int64_t)e1.size(), d2)) fail("the encoded blob is rejected");
    if (!d1.same(d2)) fail("the encoded blob decodes to other entries");
    if (encode(s, d2) != e1) fail("the second encoding differs from the first");
    return e1;
}

// Window class j of J of a sliding operator: slide J * slide, offset offset + j * slide.
static std::vector<ckpt::Spec> classes_of(const ckpt::Spec& s, int64_t J) {
    std::vector<ckpt::Spec> kids((size_t)J, s);
    for (int64_t j = 0; j < J; ++j) {
        kids[j].assigner = GW_SLIDING;
        kids[j].slide = kids[j].cfg_slide = J * s.slide;
        kids[j].offset = s.offset + j * s.slide;
    }
    return kids;
}

static void valid_blob(const int64_t* p, const uint8_t* b, int64_t len) {
    const ckpt::Spec s = spec_of(p);
    const int64_t J = p[kSpecParams];
    Decoded d;
    if (!decode(s, b, len, d)) fail("a valid blob is rejected");
    emit(round_trip(s, d));
    if (J > 0) {
        const std::vector<ckpt::Spec> kids = classes_of(s, J);
        snap::Cursor c;
        std::vector<Bytes> parts;
        if (snap::payload(b, len, d.hd, c) || ckpt::cut_classes(s, kids, d.hd, c, parts)) fail("cut_classes");
        size_t n = 0;
        for (int64_t j = 0; j < J; ++j) {  // each part restores into its class
            Decoded dj;
            if (!decode(kids[j], parts[j].data(), (int64_t)parts[j].size(), dj)) fail("a class rejects its part");
            n += dj.win.size();
        }
        if (n != d.win.size()) fail("the classes' parts hold other entries");
        snap::Writer w;
        snap::Header hd;
        if (ckpt::merge_classes(s, parts, d.hd.kg_lo, d.hd.kg_hi, w, hd)) fail("merge_classes");
        emit(w.finish(hd));
    }
    printf("ok %zu\n", d.win.size() + d.ent.size());
}

static void print_windows(const int64_t* p, const uint8_t* b, int64_t len) {
    Decoded d;
    if (!decode(spec_of(p), b, len, d)) fail("a valid blob is rejected");
    printf("windows=");
    for (const auto& e : d.win) printf("%lld:%lld:%lld:%lld,", (long long)e[0], (long long)e[1], (long long)e[2], (long long)e[4]);
    printf(" hashes=");
    for (const auto& h : d.hashes) printf("%lld:%d,", (long long)h.first, h.second);
    puts("");
}

// Every decoder, cut and tool over bytes that may be anything; only the sanitizers judge.
static void read_all(const ckpt::Spec& own, const uint8_t* b, int64_t len) {
    snap::Header hd;
    snap::Cursor c;
    const Bytes blob(b, b + len);
    if (!snap::open(b, len, 1, snap::kMaxVersion, hd, c)) {
        for (int kind = 0; kind < 4; ++kind) {
            ckpt::Spec s = own;
            s.assigner = kind == 0 ? GW_SLIDING : kind == 1 ? GW_SESSION : kind == 2 ? GW_COUNT_TUMBLING : GW_COUNT_SLIDING;
            s.slide = s.cfg_slide = s.slide > 0 ? s.slide : 300;
            s.ew = kind == 0 ? 0 : kind == 1 ? 6 : 2 + 2 * gw::cell_words(s.agg);
            ckpt::HashPairs hp;
            std::vector<int64_t> ent;
            std::vector<ckpt::WindowEntry> win;
            std::string why;
            if (kind == 0) ckpt::decode_windows(s, hd, c, win, hp, why);
            if (kind == 1) ckpt::decode_sessions(s, hd, c, ent, hp);
            if (kind == 2) ckpt::decode_count(s, hd, c, ent, hp);
            if (kind == 3) ckpt::decode_slots(s, hd, c, ent, hp);
            hp.check();
            if (kind == 0) {
                std::vector<Bytes> parts;
                snap::Writer w;
                snap::Header mh;
                if (!ckpt::cut_classes(s, classes_of(s, 3), hd, c, parts)) ckpt::merge_classes(s, parts, hd.kg_lo, hd.kg_hi, w, mh);
            }
        }
        ckpt::FirstElementSplit split;
        if (hd.flags & snap::kFirstElement) split.split(own.agg, 100, hd, c);  // as gw_restore checks first
        for (int by = 0; by < 2; ++by) {
            ckpt::FirstElementJoin join;
            snap::Writer w;
            if (!join.open(blob, by ? nullptr : &blob)) join.write(own.agg, std::vector<int64_t>(join.a.entries, 7), w);
        }
    }
    int64_t n = 0, mx = 0;
    if (!ckpt::payloads(b, len, nullptr, 0, &n, &mx)) {
        std::vector<int64_t> ps((size_t)n + 1), to((size_t)n + 1, 5);
        if (ckpt::payloads(b, len, ps.data(), n, &n, &mx)) fail("payloads: the second call differs");
        Bytes copy(b, b + len);
        if (ckpt::remap_payloads(copy.data(), len, ps.data(), to.data(), n)) fail("remap_payloads rejects what payloads read");
    }
}

static void damaged_blob(const int64_t* p, const uint8_t* b, int64_t len) {
    const ckpt::Spec s = spec_of(p);
    Decoded d;
    const bool accepted = decode(s, b, len, d);
    const std::string why = g_why;
    if (accepted) round_trip(s, d);
    read_all(s, b, len);
    int64_t out_len = 0;
    const int slice_rc = ckpt::slice(b, len, (int32_t)p[kSpecParams], nullptr, 0, &out_len).code;
    if (slice_rc == GW_OK) {
        Bytes part((size_t)out_len);
        if (ckpt::slice(b, len, (int32_t)p[kSpecParams], part.data(), out_len, &out_len)) fail("slice: the second call differs");
    }
    printf("dec=%d slice=%d keys=", (int)accepted, slice_rc);
    int64_t n = 0;
    if (ckpt::keys(b, len, nullptr, 0, &n)) {
        printf("invalid why=%s\n", why.c_str());
        return;
    }
    std::vector<int64_t> ks((size_t)n + 1), to((size_t)n + 1);
    if (ckpt::keys(b, len, ks.data(), n, &n)) fail("keys: the second call differs");
    for (int64_t i = 0; i < n; ++i) {
        printf(i ? ",%lld" : "%lld", (long long)ks[i]);
        to[i] = ks[i] ^ 1;
    }
    printf(" why=%s\n", why.c_str());
    Bytes copy(b, b + len);
    if (ckpt::remap_keys(copy.data(), len, ks.data(), to.data(), n)) fail("remap_keys rejects what keys read");
    if (ckpt::keys(copy.data(), len, nullptr, 0, &n)) fail("the remapped blob is rejected");
}

// Sliding 900 / 300 (n = 3, m = 1), sum_i64, max parallelism 4.  Key A: pane 0 = 5, pane 1 =
// 7 and 11 (two cells: the fold).  Key B: pane 5 = 100 and the restored window 4 = 1000 with
// its timer pending.
static void pane_case(const int64_t* p) {
    ckpt::Spec s{};
    s.agg = GW_SUM_I64; s.assigner = GW_SLIDING; s.trigger = GW_EVENT_TIME_TRIGGER; s.max_parallelism = 4;
    s.size = 900; s.slide = s.cfg_slide = 300; s.allowed_lateness = p[4];
    s.n = 3; s.m = 1;
    const int64_t A = p[0], B = p[1];
    const ckpt::KeyHashes kh;
    const std::vector<int64_t> col[4] = {{B, A, A, A}, {5, 1, 0, 1}, {100, 7, 5, 11}, {0, 0, 0, 0}};
    std::vector<int32_t> kgs;
    for (int64_t key : col[0]) kgs.push_back(kh.key_group(key, 4));
    const std::vector<ckpt::WindowEntry> ov = {{B, 4, 1000, 0, ckpt::kTimer}};
    snap::Writer w;
    snap::Header hd;
    if (ckpt::encode_windows(s, kh, 0, 3, col, kgs, ov, (i128)p[2], (i128)p[3], w, hd)) fail("encode_windows");
    emit(w.finish(hd));
    puts("ok");
}

// Two key groups: (key 3: windows [0, 10) and [10, 20)), then (key 9: window [0, 10)); sum_i64
// with key hashes; payloads 70, 71, 72; a timer per window.
static void first_element_case() {
    ckpt::Spec s{};
    s.agg = GW_SUM_I64; s.assigner = GW_TUMBLING; s.max_parallelism = 8;
    s.size = s.slide = s.cfg_slide = 10;
    ckpt::KeyHashes kh;
    kh.kv = {{3, 33}, {9, 99}};
    snap::Writer w;
    ckpt::Group grp;
    const int64_t rows[3][4] = {{3, 0, 500, 70}, {3, 10, 501, 71}, {9, 0, 502, 72}};  // key, start, sum, payload
    for (int i = 0; i < 3; ++i) {
        grp.state(s, kh, rows[i][1], rows[i][1] + 10, rows[i][0], rows[i][2], 0);
        snap::put64(grp.st, rows[i][3]);
        grp.window_timers(s, true, rows[i][0], rows[i][1], rows[i][1] + 10);
        if (i >= 1) grp.end(w);
    }
    snap::Header hd = s.header(4, 2, 3, true);
    hd.flags |= snap::kFirstElement;
    const Bytes blob = w.finish(hd);
    snap::Header got;
    snap::Cursor c;
    ckpt::FirstElementSplit split;
    if (snap::open(blob.data(), (int64_t)blob.size(), 4, 4, got, c) || split.split(s.agg, 100, got, c)) fail("split");
    if (split.pays != std::vector<int64_t>{70, 71, 72} || split.max_end != 20) fail("split: payloads");
    if (split.by_cols[0] != std::vector<int64_t>{3, 3, 9} || split.by_cols[1] != std::vector<int64_t>{0, 10, 0} ||
        split.by_cols[2] != std::vector<int64_t>{500, 501, 502})
        fail("split: columns");
    ckpt::Spec seq = s;  // the second operator: MIN of the sequence
    seq.agg = GW_MIN_I64;
    Decoded da, db;
    if (!decode(s, split.blobs[0].data(), (int64_t)split.blobs[0].size(), da)) fail("the first operator rejects its blob");
    if (!decode(seq, split.blobs[1].data(), (int64_t)split.blobs[1].size(), db)) fail("the second operator rejects its blob");
    if (da.win != std::vector<std::array<int64_t, 5>>{{3, 0, 500, 0, 1}, {3, 1, 501, 0, 1}, {9, 0, 502, 0, 1}}) fail("split: entries");
    if (db.win != std::vector<std::array<int64_t, 5>>{{3, 0, 100, 0, 1}, {3, 1, 101, 0, 1}, {9, 0, 102, 0, 1}}) fail("split: sequences");
    ckpt::FirstElementJoin join;
    if (join.open(split.blobs[0], &split.blobs[1]) || join.seqs != std::vector<int64_t>{100, 101, 102}) fail("join");
    snap::Writer back;
    const snap::Header bh = join.write(s.agg, split.pays, back);
    if (back.finish(bh) != blob) fail("the joined blob differs from the input");
    ckpt::FirstElementJoin by;  // minBy / maxBy: one operator
    if (by.open(split.blobs[0], nullptr) || by.by_key != split.by_cols[0] || by.by_start != split.by_cols[1] ||
        by.by_res != split.by_cols[2])
        fail("join: minBy / maxBy columns");
    puts("ok");
}

int main(int argc, char** argv) {
    FILE* f = argc > 2 ? fopen(argv[1], "rb") : nullptr;
    g_out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (!f || !g_out) return 2;
    int64_t kind, np, len;
    while (fread(&kind, 8, 1, f) == 1) {
        if (fread(&np, 8, 1, f) != 1 || np < 0 || np > 64) return 2;
        std::vector<int64_t> p((size_t)np + 1);
        if (np && fread(p.data(), 8, (size_t)np, f) != (size_t)np) return 2;
        if (fread(&len, 8, 1, f) != 1 || len < 0) return 2;
        std::unique_ptr<uint8_t[]> blob(new uint8_t[(size_t)len]);
        if (len && fread(blob.get(), (size_t)len, 1, f) != 1) return 2;
        if (kind == 0) valid_blob(p.data(), blob.get(), len);
        if (kind == 1) print_windows(p.data(), blob.get(), len);
        if (kind == 2) damaged_blob(p.data(), blob.get(), len);
        if (kind == 3) pane_case(p.data());
        if (kind == 4) first_element_case();
    }
    fclose(f);
    fclose(g_out);
    return 0;
}
