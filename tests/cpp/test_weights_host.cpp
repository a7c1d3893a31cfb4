// The checkpoint readers behind mi_clip_load / mi_clip_load_text / mi_weights_list (image_search_amd/csrc/weights.h) as a
// stand-alone program: the half / bfloat16 conversions over all 65 536 bit patterns against arithmetic written here, valid
// safetensors files and Burn records read back value by value, and a deterministic corpus of broken files — every
// truncation, single-byte corruption of the structure, and hostile cases written out by name.  Every broken file must end in
// mi::Error with MI_ERR_IO or MI_ERR_UNSUPPORTED, or be read: no other exception, no sanitizer report, under a second.
// Built with -fsanitize=address,undefined and run with ASAN_OPTIONS=max_allocation_size_mb=64 (tests/test_weights_host.py):
// the files are a few KB, so a buffer sized from a count in the file instead of the bytes present ends the run.
//
//   test_weights_host <scratch dir>          leaves hostile_*.bin and hostile.txt ("<file> <accept|refuse|any>") there
//   test_weights_host <scratch dir> <name>   only the hostile cases whose name contains <name>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../image_search_amd/csrc/weights.h"

using namespace mi;

static int failures = 0;
#define EXPECT(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

typedef std::string Bytes;

static void write_file(const std::string& path, const Bytes& b) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) { std::printf("cannot write %s\n", path.c_str()); std::exit(2); }
    if (!b.empty() && std::fwrite(b.data(), 1, b.size(), f) != b.size()) { std::printf("short write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

// ---- the conversions, written from the formats' definitions (sign, exponent, mantissa -> ldexp) ----------------------------
static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float float_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }

static uint32_t half_bits(uint16_t h) {   // IEEE binary16: 1 + 5 + 10, bias 15
    const uint32_t sign = (uint32_t)(h >> 15) << 31;
    const int ex = (h >> 10) & 31, man = h & 1023;
    if (ex == 31) return sign | 0x7f800000u | ((uint32_t)man << 13);   // inf; NaN keeps its payload in the top mantissa bits
    const float mag = ex == 0 ? std::ldexp((float)man, -24) : std::ldexp((float)(1024 + man), ex - 25);
    return sign | bits_of(mag);
}
static uint32_t bf16_bits(uint16_t h) {   // bfloat16: 1 + 8 + 7, bias 127
    const uint32_t sign = (uint32_t)(h >> 15) << 31;
    const int ex = (h >> 7) & 255, man = h & 127;
    if (ex == 255) return sign | 0x7f800000u | ((uint32_t)man << 16);
    const float mag = ex == 0 ? std::ldexp((float)man, -133) : std::ldexp((float)(128 + man), ex - 134);
    return sign | bits_of(mag);
}
static uint32_t expect_bits(uint16_t h, const std::string& dtype) { return dtype == "F16" ? half_bits(h) : bf16_bits(h); }

static void conversions() {
    std::vector<uint16_t> all(65536);
    for (uint32_t i = 0; i < 65536; ++i) all[i] = (uint16_t)i;
    std::vector<float> out(65536);
    for (const char* dt : {"F16", "BF16"}) {
        to_f32(all.data(), dt, 65536, out.data(), "all");
        int bad = 0;
        for (uint32_t i = 0; i < 65536; ++i) bad += bits_of(out[i]) != expect_bits((uint16_t)i, dt);
        if (bad) std::printf("%s: %d of 65536 patterns differ\n", dt, bad);
        EXPECT(bad == 0);
    }
    // the named corners, against constants
    const uint16_t h[] = {0x0000, 0x8000, 0x0001, 0x83ff, 0x0400, 0x3c00, 0x7bff, 0x7c00, 0xfc00, 0x7e00, 0xfd55};
    const uint32_t hf[] = {0x00000000u, 0x80000000u, 0x33800000u, 0xb87fc000u, 0x38800000u, 0x3f800000u, 0x477fe000u, 0x7f800000u,
                           0xff800000u, 0x7fc00000u, 0xffaaa000u};
    to_f32(h, "F16", 11, out.data(), "corners");
    for (int i = 0; i < 11; ++i) EXPECT(bits_of(out[i]) == hf[i]);
    const uint16_t b[] = {0x0000, 0x8000, 0x0001, 0x807f, 0x0080, 0x3f80, 0x7f7f, 0x7f80, 0xff80, 0x7fc0, 0xffd5};
    to_f32(b, "BF16", 11, out.data(), "corners");
    for (int i = 0; i < 11; ++i) EXPECT(bits_of(out[i]) == (uint32_t)b[i] << 16);
    EXPECT(std::isnan(out[9]) && std::isnan(out[10]) && std::signbit(out[10]) && std::isinf(out[7]) && out[8] < 0);
    const float f[3] = {1.5f, -0.0f, 3e38f};
    to_f32(f, "F32", 3, out.data(), "f32");
    EXPECT(std::memcmp(out.data(), f, 12) == 0);
    for (const char* dt : {"I64", "F64", "f16", "", "F8_E4M3"}) {
        int code = 0;
        try { to_f32(h, dt, 1, out.data(), "x"); } catch (const Error& e) { code = e.code; }
        EXPECT(code == MI_ERR_UNSUPPORTED);
    }
}

// ---- builders ------------------------------------------------------------------------------------------------------------
static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// n 16-bit patterns that are finite in either format (the exponent fields are never all ones), zeros and subnormals included
static std::vector<uint16_t> patterns(uint64_t seed, size_t n) {
    std::vector<uint16_t> v(n);
    for (size_t i = 0; i < n; ++i) {
        uint16_t p = (uint16_t)mix(seed * 1000003 + i);
        if (((p >> 10) & 31) == 31) p &= (uint16_t)~0x0400;
        if (((p >> 7) & 255) == 255) p &= (uint16_t)~0x0080;
        if (i % 17 == 3) p &= 0x8000;            // +-0
        if (i % 17 == 5) p &= 0x803f;            // subnormal in both
        v[i] = p;
    }
    return v;
}
static Bytes le16(const std::vector<uint16_t>& v) {
    Bytes b;
    for (uint16_t x : v) { b.push_back((char)(x & 255)); b.push_back((char)(x >> 8)); }
    return b;
}
static Bytes le64(uint64_t v) { Bytes b; for (int i = 0; i < 8; ++i) b.push_back((char)((v >> (8 * i)) & 255)); return b; }
static Bytes safetensors(const std::string& header, const Bytes& data) { return le64(header.size()) + header + data; }

struct Mp {   // a MessagePack writer
    Bytes b;
    void raw(std::initializer_list<int> l) { for (int x : l) b.push_back((char)x); }
    void be(uint64_t v, int n) { for (int i = n - 1; i >= 0; --i) b.push_back((char)((v >> (8 * i)) & 255)); }
    void nil() { raw({0xc0}); }
    void map(size_t n) { if (n < 16) raw({(int)(0x80 | n)}); else { raw({0xde}); be(n, 2); } }
    void arr(size_t n) { if (n < 16) raw({(int)(0x90 | n)}); else if (n < 65536) { raw({0xdc}); be(n, 2); } else { raw({0xdd}); be(n, 4); } }
    void str(const std::string& s) { if (s.size() < 32) raw({(int)(0xa0 | s.size())}); else { raw({0xd9, (int)s.size()}); } b += s; }
    void bin(const Bytes& d) { if (d.size() < 256) raw({0xc4, (int)d.size()}); else if (d.size() < 65536) { raw({0xc5}); be(d.size(), 2); } else { raw({0xc6}); be(d.size(), 4); } b += d; }
    void u(uint64_t v) { if (v < 128) raw({(int)v}); else if (v < 256) raw({0xcc, (int)v}); else if (v < 65536) { raw({0xcd}); be(v, 2); } else if (v < (1ull << 32)) { raw({0xce}); be(v, 4); } else { raw({0xcf}); be(v, 8); } }
    void f32(float f) { raw({0xca}); be(bits_of(f), 4); }
};

struct Tensor {   // in the Hugging Face convention: Linear weights [out, in]
    std::string name, dtype;
    std::vector<int64_t> shape;
    std::vector<uint16_t> bits;
    size_t n() const { size_t p = 1; for (auto d : shape) p *= (size_t)d; return p; }
    float value(size_t i) const { return float_of(expect_bits(bits[i], dtype)); }
};
enum Form { BIN, U8_ARRAY, LEGACY_VALUE };

// A CLIP vision tower of D 8, FF 16, E 4, 5 positions, 1 x 1 patches, `layers` layers, as burn-import would record it: field names in
// graph order, LayerNorm modules, Linear modules with the weight kept [in, out].  Returns the file; `want` gets the tensors
// under the names and in the shapes the reader must give them.
static const int TD = 8, TFF = 16, TE = 4, TS = 5;
// `bias_moved`: fc2 of the last layer has no bias and the projection has one of D elements — every count of the inventory still fits
static Bytes burn_tower(Form form, int layers, std::vector<Tensor>& want, uint64_t seed = 1, bool bias_moved = false) {
    want.clear();
    int serial = 0;
    auto make = [&](const std::string& name, std::vector<int64_t> shape) {
        Tensor t;
        t.name = name; t.shape = shape; t.dtype = (serial % 2) ? "BF16" : "F16";
        t.bits = patterns(seed * 100 + (uint64_t)serial, t.n());
        ++serial;
        want.push_back(t);
        return t;
    };
    Mp m;
    auto tensor = [&](const Tensor& t, std::vector<int64_t> stored_shape, bool transposed) {
        std::vector<uint16_t> d = t.bits;
        if (transposed) {
            const size_t rows = (size_t)t.shape[0], cols = (size_t)t.shape[1];
            for (size_t o = 0; o < rows; ++o) for (size_t i = 0; i < cols; ++i) d[i * rows + o] = t.bits[o * cols + i];
        }
        m.map(2);   // {"id", "param"}
        m.str("id"); m.str(std::to_string(serial));
        m.str("param");
        m.map(form == LEGACY_VALUE ? 2 : 3);
        if (form == LEGACY_VALUE) {
            m.str("value"); m.arr(d.size());
            for (uint16_t x : d) m.f32(float_of(expect_bits(x, t.dtype)));
        } else {
            m.str("bytes");
            const Bytes raw = le16(d);
            if (form == BIN) m.bin(raw);
            else { m.arr(raw.size()); for (char c : raw) m.u((uint8_t)c); }
        }
        m.str("shape"); m.arr(stored_shape.size());
        for (auto s : stored_shape) m.u((uint64_t)s);
        if (form != LEGACY_VALUE) { m.str("dtype"); m.str(t.dtype); }
    };
    int n_lin = 0, n_ln = 0;
    const std::string v = "vision_model.";
    auto ln = [&](const std::string& prefix) {
        m.str("layernormalization" + std::to_string(++n_ln));
        m.map(3);
        m.str("gamma"); tensor(make(prefix + ".weight", {TD}), {TD}, false);
        m.str("beta"); tensor(make(prefix + ".bias", {TD}), {TD}, false);
        m.str("epsilon"); m.f32(1e-5f);
    };
    auto linear = [&](const std::string& prefix, int d_out, int d_in, bool bias) {
        m.str("linear" + std::to_string(++n_lin));
        m.map(2);
        m.str("weight"); tensor(make(prefix + ".weight", {d_out, d_in}), {d_in, d_out}, true);
        m.str("bias");
        if (bias) tensor(make(prefix + ".bias", {d_out == TE ? TD : d_out}), {d_out == TE ? TD : d_out}, false); else m.nil();
    };
    m.map(2);
    m.str("metadata"); m.map(2); m.str("float"); m.str("f16"); m.str("version"); m.str("0.19.1");
    m.str("item");
    m.map((size_t)(1 + 2 + 1 + 8 * layers + 1 + 1));
    m.str("conv2d1"); m.map(2);
    m.str("weight"); tensor(make(v + "embeddings.patch_embedding.weight", {TD, 3, 1, 1}), {TD, 3, 1, 1}, false);
    m.str("bias"); m.nil();
    // the reader files the position table second and the class embedding third, whatever their order in the record
    Tensor pos = make(v + "embeddings.position_embedding.weight", {TS, TD}), cls = make(v + "embeddings.class_embedding", {TD});
    m.str("constant1"); tensor(cls, {1, 1, TD}, false);
    m.str("constant2"); tensor(pos, {1, TS, TD}, false);
    ln(v + "pre_layrnorm");
    for (int l = 0; l < layers; ++l) {
        const std::string p = v + "encoder.layers." + std::to_string(l) + ".";
        ln(p + "layer_norm1");
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) linear(p + "self_attn." + n, TD, TD, true);
        ln(p + "layer_norm2");
        linear(p + "mlp.fc1", TFF, TD, true);
        linear(p + "mlp.fc2", TD, TFF, !(bias_moved && l + 1 == layers));
    }
    ln(v + "post_layernorm");
    linear("visual_projection", TE, TD, bias_moved);
    return m.b;
}

// ---- what every file goes through ----------------------------------------------------------------------------------------------
enum Outcome { READ, REFUSED, WRONG };
static double slowest = 0;
static std::string slowest_case;
// open, list, and read every tensor; anything but success or mi::Error{MI_ERR_IO, MI_ERR_UNSUPPORTED} is WRONG
static Outcome probe(const std::string& path, const std::string& label, std::string* why = nullptr) {
    const auto t0 = std::chrono::steady_clock::now();
    Outcome o = READ;
    try {
        const std::unique_ptr<WeightFile> f = open_weights(path.c_str());
        for (const std::string& name : f->names()) {
            const TensorInfo& t = f->info(name);
            if (!f->has(name)) { o = WRONG; if (why) *why = "a listed tensor is not there"; }
            try {
                const std::vector<float> data = f->read(name, t.numel());
                if ((int64_t)data.size() != t.numel()) { o = WRONG; if (why) *why = "read returned another size"; }
            } catch (const Error& e) {   // a listed tensor may be unreadable (an integer dtype, for one) — by code
                if (e.code != MI_ERR_IO && e.code != MI_ERR_UNSUPPORTED) { o = WRONG; if (why) *why = e.what(); }
            }
        }
        (void)f->skipped_lines();
    } catch (const Error& e) {
        o = (e.code == MI_ERR_IO || e.code == MI_ERR_UNSUPPORTED) ? REFUSED : WRONG;
        if (why) *why = e.what();
    } catch (const std::exception& e) {
        o = WRONG;
        if (why) *why = std::string("not mi::Error: ") + e.what();
    } catch (...) {
        o = WRONG;
        if (why) *why = "not a std::exception";
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (dt > slowest) { slowest = dt; slowest_case = label; }
    if (dt > 1.0) { std::printf("FAILED: %s took %.2f s\n", label.c_str(), dt); ++failures; }
    return o;
}

// ---- 2. valid files ---------------------------------------------------------------------------------------------------------
static Bytes small_safetensors(std::vector<Tensor>* want = nullptr, size_t* header_bytes = nullptr) {
    Tensor a, b, c, d;
    a.name = "a.f32"; a.dtype = "F32"; a.shape = {2, 3};
    b.name = "b \"quoted\" \\ name"; b.dtype = "F16"; b.shape = {5}; b.bits = patterns(7, 5);
    c.name = "c.bf16"; c.dtype = "BF16"; c.shape = {3, 2}; c.bits = patterns(8, 6);
    d.name = "d.empty"; d.dtype = "F16"; d.shape = {0, 4};
    const float af[6] = {1.0f, -2.5f, 3e-40f, -0.0f, 65504.0f, 1e30f};
    Bytes data((const char*)af, 24);
    data += le16(b.bits) + le16(c.bits);
    const std::string h =
        "{\"__metadata__\":{\"num_attention_heads\":\"2\",\"format\":\"pt\"},"
        "\"a.f32\":{\"dtype\":\"F32\",\"shape\":[2,3],\"data_offsets\":[0,24]},"
        "\"b \\\"quoted\\\" \\\\ name\":{\"dtype\":\"F16\",\"shape\":[5],\"data_offsets\":[24,34]},"
        "\"c.bf16\":{\"extra\":{\"x\":[1,[2,{\"y\":[]},\"s]\"],-3.5e2,true,null],\"z\":{}},\"dtype\":\"BF16\",\"shape\":[3,2],\"data_offsets\":[34,46]},"
        "\"d.empty\":{\"dtype\":\"F16\",\"shape\":[0,4],\"data_offsets\":[46,46]}}  ";
    if (want) {
        *want = {a, b, c, d};
        (*want)[0].bits.clear();
    }
    if (header_bytes) *header_bytes = 8 + h.size();
    return safetensors(h, data);
}

static void valid_files(const std::string& dir) {
    const std::string p = dir + "/valid.bin";
    {
        std::vector<Tensor> want;
        write_file(p, small_safetensors(&want));
        const std::unique_ptr<WeightFile> f = open_weights(p.c_str());
        EXPECT(f->meta.size() == 2 && f->meta["num_attention_heads"] == "2" && f->meta["format"] == "pt");
        const std::vector<std::string> names = f->names();
        EXPECT(names.size() == 4);
        for (size_t i = 0; i < want.size() && i < names.size(); ++i) {
            EXPECT(names[i] == want[i].name && f->has(want[i].name));
            const TensorInfo& t = f->info(names[i]);
            EXPECT(t.dtype == want[i].dtype && t.shape == want[i].shape && t.numel() == (int64_t)want[i].n());
            const std::vector<float> got = f->read(names[i], t.numel());
            EXPECT(got.size() == want[i].n());
            if (i == 0) {
                const float af[6] = {1.0f, -2.5f, 3e-40f, -0.0f, 65504.0f, 1e30f};
                EXPECT(got.size() == 6 && std::memcmp(got.data(), af, 24) == 0);
            } else
                for (size_t j = 0; j < got.size(); ++j) EXPECT(bits_of(got[j]) == expect_bits(want[i].bits[j], want[i].dtype));
        }
        EXPECT(!f->has("nope"));
        int code = 0;
        try { f->read("a.f32", 5); } catch (const Error& e) { code = e.code; }   // the caller's element count is checked
        EXPECT(code == MI_ERR_IO);
        code = 0;
        try { f->info("nope"); } catch (const Error& e) { code = e.code; }
        EXPECT(code == MI_ERR_IO);
    }
    for (Form form : {BIN, U8_ARRAY, LEGACY_VALUE})
        for (int layers : {1, 2}) {
            std::vector<Tensor> want;
            write_file(p, burn_tower(form, layers, want, 3 + (uint64_t)form));
            const std::unique_ptr<WeightFile> f = open_weights(p.c_str());
            EXPECT(f->meta["burn.float"] == "f16");
            const std::vector<std::string> names = f->names();
            EXPECT(names.size() == want.size() && want.size() == (size_t)(3 + 2 + 16 * layers + 2 + 1));
            EXPECT(f->skipped_lines().empty());
            size_t found = 0;
            for (const Tensor& w : want) {
                if (!f->has(w.name)) { std::printf("missing %s\n", w.name.c_str()); continue; }
                ++found;
                const TensorInfo& t = f->info(w.name);
                EXPECT(t.shape == w.shape);
                EXPECT(t.dtype == (form == LEGACY_VALUE ? "F32" : w.dtype));
                const std::vector<float> got = f->read(w.name, (int64_t)w.n());
                EXPECT(got.size() == w.n());
                size_t bad = 0;
                for (size_t j = 0; j < got.size() && j < w.n(); ++j) bad += bits_of(got[j]) != expect_bits(w.bits[j], w.dtype);
                if (bad) std::printf("%s: %zu values differ (form %d)\n", w.name.c_str(), bad, (int)form);
                EXPECT(bad == 0);
            }
            EXPECT(found == want.size());
            // a Linear kept [in, out] came back [out, in]: fc1 is [FF, D] and not symmetric
            EXPECT((f->info("vision_model.encoder.layers.0.mlp.fc1.weight").shape == std::vector<int64_t>{TFF, TD}));
        }
}

// ---- 3. every truncation, 4. single-byte corruption of the structure ----------------------------------------------------
static void corpus(const std::string& dir) {
    const std::string p = dir + "/corpus.bin";
    std::vector<Tensor> want;
    size_t header = 0;
    const Bytes st = small_safetensors(nullptr, &header), mpk = burn_tower(BIN, 1, want);
    std::printf("corpus: safetensors %zu bytes (header %zu), record %zu bytes\n", st.size(), header, mpk.size());
    long read = 0, refused = 0;
    auto run = [&](const Bytes& b, const std::string& label) {
        write_file(p, b);
        std::string why;
        const Outcome o = probe(p, label, &why);
        if (o == WRONG) { std::printf("FAILED: %s: %s\n", label.c_str(), why.c_str()); ++failures; }
        (o == READ ? read : refused) += 1;
    };
    for (const Bytes* file : {&st, &mpk})
        for (size_t len = 0; len < file->size(); ++len) {
            run(file->substr(0, len), std::string(file == &st ? "safetensors" : "record") + " cut at " + std::to_string(len));
        }
    // a truncated file is never read as if it were whole
    EXPECT(read == 0);
    const int with[] = {0x00, 0x7f, 0x80, 0xff, 0x5b, 0x7b, 0x22, 0x2d, 0xc1, 0xc6, 0xcf, 0xd3, 0xdd, 0xdf};
    for (const Bytes* file : {&st, &mpk}) {
        const size_t span = file == &st ? header : std::min<size_t>(512, file->size());
        for (size_t at = 0; at < span; ++at)
            for (int v : with) {
                if ((unsigned char)(*file)[at] == v) continue;
                Bytes b = *file;
                b[at] = (char)v;
                run(b, std::string(file == &st ? "safetensors" : "record") + " byte " + std::to_string(at) + " = " + std::to_string(v));
            }
    }
    std::printf("corpus: %ld files read, %ld refused\n", read, refused);
}

// ---- 5. hostile cases, each by name --------------------------------------------------------------------------------------------
struct Case { std::string name; Bytes file; const char* expect; };   // "accept", "refuse" or "any"

static std::string one_tensor(const std::string& fields) { return "{\"t\":{" + fields + "}}"; }
static Bytes st_case(const std::string& fields, size_t data = 8) { return safetensors(one_tensor(fields), Bytes(data, '\1')); }
// {"item": {"vision_model.t": <tensor map written by `body`>}} — a record that carries its own names
static Bytes mpk_case(const std::function<void(Mp&)>& body) {
    Mp m;
    m.map(1); m.str("item"); m.map(1); m.str("vision_model.t");
    body(m);
    return m.b;
}

static std::vector<Case> hostile_cases() {
    std::vector<Case> c;
    const std::string ok_fields = "\"dtype\":\"F32\",\"shape\":[2],\"data_offsets\":[0,8]";
    c.push_back({"control_safetensors", st_case(ok_fields), "accept"});
    c.push_back({"control_record", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.u(2); m.str("dtype"); m.str("F32"); }), "accept"});
    // nesting
    c.push_back({"nesting_2000000_brackets", st_case(ok_fields + ",\"x\":" + std::string(2000000, '[')), "refuse"});
    {
        std::string s;
        s.reserve(10000000);
        for (int i = 0; i < 2000000; ++i) s += "{\"a\":";
        c.push_back({"nesting_2000000_objects", st_case(ok_fields + ",\"x\":" + s), "refuse"});
    }
    c.push_back({"nesting_64_json_accepted", st_case(ok_fields + ",\"x\":" + std::string(64, '[') + std::string(64, ']')), "accept"});
    c.push_back({"nesting_65_json_refused", st_case(ok_fields + ",\"x\":" + std::string(65, '[') + std::string(65, ']')), "refuse"});
    for (int depth : {64, 65}) {   // arrays below the top-level map of a record
        Mp m;
        m.map(2);
        m.str("vision_model.t"); m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.u(2); m.str("dtype"); m.str("F32");
        m.str("deep");
        for (int i = 0; i < depth - 1; ++i) m.arr(1);
        m.arr(0);
        c.push_back({depth == 64 ? "nesting_64_msgpack_accepted" : "nesting_65_msgpack_refused", m.b, depth == 64 ? "accept" : "refuse"});
    }
    // header length
    c.push_back({"header_length_0", le64(0) + one_tensor(ok_fields) + Bytes(8, '\1'), "refuse"});
    c.push_back({"header_length_past_the_file", le64(4096) + one_tensor(ok_fields) + Bytes(8, '\1'), "refuse"});
    c.push_back({"header_length_above_256MiB", le64((256ull << 20) + 8) + one_tensor(ok_fields) + Bytes(8, '\1'), "refuse"});
    c.push_back({"header_length_2_to_64_minus_1", le64(~0ull) + one_tensor(ok_fields) + Bytes(8, '\1'), "refuse"});
    // data_offsets
    auto offs = [&](const std::string& o) { return st_case("\"dtype\":\"F32\",\"shape\":[2],\"data_offsets\":" + o); };
    c.push_back({"offsets_begin_above_end", offs("[8,0]"), "refuse"});
    c.push_back({"offsets_end_past_the_file", offs("[0,16]"), "refuse"});
    c.push_back({"offsets_negative", offs("[-8,0]"), "refuse"});
    c.push_back({"offsets_negative_end", offs("[0,-8]"), "refuse"});
    c.push_back({"offsets_2_to_63", offs("[0,9223372036854775808]"), "refuse"});
    c.push_back({"offsets_sum_with_the_data_start_wraps", offs("[18446744073709551544,18446744073709551552]"), "refuse"});
    c.push_back({"offsets_sum_wraps_in_int64", offs("[9223372036854775799,9223372036854775807]"), "refuse"});
    // shapes
    auto shape = [&](const std::string& s, const std::string& o) { return st_case("\"dtype\":\"F32\",\"shape\":" + s + ",\"data_offsets\":" + o); };
    c.push_back({"shape_negative_dimension", shape("[-2]", "[0,8]"), "refuse"});
    c.push_back({"shape_two_negative_dimensions", shape("[-1,-2]", "[0,8]"), "refuse"});
    c.push_back({"shape_zero_dimension", shape("[0,7]", "[0,0]"), "accept"});
    c.push_back({"shape_dimension_2_to_31", shape("[2147483648]", "[0,8]"), "refuse"});
    c.push_back({"shape_product_above_2_to_63", shape("[2147483647,2147483647,2147483647]", "[0,8]"), "refuse"});
    c.push_back({"shape_product_just_below_2_to_63", shape("[2147483647,2147483647,2]", "[0,8]"), "refuse"});
    c.push_back({"shape_byte_count_wraps_to_the_byte_size", shape("[1073741824,1073741824,4]", "[0,0]"), "refuse"});   // 2^62 x 4 = 2^64
    auto mpk_shape = [&](std::vector<uint64_t> dims) {
        return mpk_case([dims](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(dims.size()); for (auto d : dims) m.u(d); m.str("dtype"); m.str("F32"); });
    };
    c.push_back({"record_shape_2_to_40_squared", mpk_shape({1ull << 40, 1ull << 40}), "refuse"});
    c.push_back({"record_shape_product_above_2_to_63", mpk_shape({2147483647, 2147483647, 2147483647}), "refuse"});
    c.push_back({"record_shape_product_2_to_63", mpk_shape({1073741824, 1073741824, 4, 2}), "refuse"});
    c.push_back({"record_byte_count_wraps_to_the_byte_size", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes()); m.str("shape"); m.arr(3); m.u(1073741824); m.u(1073741824); m.u(4); m.str("dtype"); m.str("F32"); }), "refuse"});
    c.push_back({"record_shape_dimension_2_to_31", mpk_shape({2147483648ull}), "refuse"});
    c.push_back({"record_shape_negative_dimension", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.raw({0xfe}); m.str("dtype"); m.str("F32"); }), "refuse"});
    c.push_back({"record_shape_zero_dimension", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes()); m.str("shape"); m.arr(2); m.u(0); m.u(7); m.str("dtype"); m.str("F16"); }), "accept"});
    c.push_back({"record_unknown_dtype_of_2_to_60_elements", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(2); m.u(1073741824); m.u(1073741824); m.str("dtype"); m.str("Q8"); }), "any"});
    c.push_back({"record_empty_value_array", mpk_case([](Mp& m) { m.map(2); m.str("value"); m.arr(0); m.str("shape"); m.arr(1); m.u(0); }), "accept"});
    // names and dtypes
    c.push_back({"duplicate_tensor_names", safetensors("{\"t\":{" + ok_fields + "},\"t\":{\"dtype\":\"F32\",\"shape\":[1],\"data_offsets\":[0,4]}}", Bytes(8, '\1')), "refuse"});
    c.push_back({"dtype_not_a_string", st_case("\"dtype\":7,\"shape\":[2],\"data_offsets\":[0,8]"), "refuse"});
    c.push_back({"byte_size_not_shape_times_element_size", st_case("\"dtype\":\"F32\",\"shape\":[2],\"data_offsets\":[0,4]"), "refuse"});
    c.push_back({"byte_size_not_shape_times_element_size_f16", st_case("\"dtype\":\"F16\",\"shape\":[3],\"data_offsets\":[0,8]"), "refuse"});
    c.push_back({"record_byte_size_not_shape_times_element_size", mpk_case([](Mp& m) { m.map(3); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.u(3); m.str("dtype"); m.str("BF16"); }), "refuse"});
    c.push_back({"tensor_without_fields", safetensors("{\"t\":{}}", Bytes(8, '\1')), "refuse"});
    c.push_back({"unknown_dtype_listed_not_read", st_case("\"dtype\":\"I64\",\"shape\":[1],\"data_offsets\":[0,8]"), "accept"});
    // MessagePack counts of 2^32 - 1 with nothing behind them
    for (auto kv : {std::make_pair("str32", 0xdb), std::make_pair("bin32", 0xc6), std::make_pair("array32", 0xdd), std::make_pair("map32", 0xdf)}) {
        Mp m;
        m.map(1); m.str("item"); m.raw({kv.second, 0xff, 0xff, 0xff, 0xff});
        c.push_back({std::string("count_") + kv.first + "_of_2_to_32_minus_1", m.b, "refuse"});
    }
    c.push_back({"count_map32_of_2_to_32_minus_1_at_the_top", Bytes("\xdf\xff\xff\xff\xff", 5) + Bytes(8, '\0'), "refuse"});
    c.push_back({"count_shape_array32_of_2_to_32_minus_1", mpk_case([](Mp& m) { m.map(2); m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.raw({0xdd, 0xff, 0xff, 0xff, 0xff}); }), "refuse"});
    // MessagePack values
    c.push_back({"value_array_announces_2_to_32_minus_1_floats", mpk_case([](Mp& m) { m.map(2); m.str("shape"); m.arr(1); m.u(0xffffffffull); m.str("value"); m.raw({0xdd, 0xff, 0xff, 0xff, 0xff}); }), "refuse"});
    c.push_back({"bytes_array_announces_2_to_32_minus_1_bytes", mpk_case([](Mp& m) { m.map(2); m.str("shape"); m.arr(1); m.u(2); m.str("bytes"); m.raw({0xdd, 0xff, 0xff, 0xff, 0xff}); }), "refuse"});
    c.push_back({"bytes_array_holds_a_value_above_255", mpk_case([](Mp& m) { m.map(3); m.str("shape"); m.arr(1); m.u(1); m.str("dtype"); m.str("F16"); m.str("bytes"); m.arr(2); m.u(300); m.u(1); }), "refuse"});
    c.push_back({"reserved_type_byte_c1", [] { Mp m; m.map(1); m.str("item"); m.raw({0xc1}); m.b += Bytes(8, '\0'); return m.b; }(), "refuse"});
    c.push_back({"reserved_type_byte_c1_as_a_tensor_key", mpk_case([](Mp& m) { m.map(3); m.raw({0xc1}); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.u(2); m.str("bytes"); m.bin(Bytes(8, '\1')); }), "refuse"});
    for (int ext : {0xd4, 0xd8, 0xc7}) {   // fixext 1, fixext 16, ext 8 where a key belongs
        Mp m;
        m.map(2);
        if (ext == 0xc7) m.raw({0xc7, 3, 5, 1, 2, 3}); else { m.raw({ext, 5}); m.b += Bytes(ext == 0xd4 ? 1 : 16, '\2'); }
        m.u(1);
        m.str("vision_model.t"); m.map(4);
        if (ext == 0xc7) m.raw({0xc7, 3, 5, 1, 2, 3}); else { m.raw({ext, 5}); m.b += Bytes(ext == 0xd4 ? 1 : 16, '\2'); }
        m.nil();
        m.str("bytes"); m.bin(Bytes(8, '\1')); m.str("shape"); m.arr(1); m.u(2); m.str("dtype"); m.str("F32");
        c.push_back({"ext_type_" + std::to_string(ext) + "_in_key_position", m.b, "accept"});
    }
    c.push_back({"ext32_length_of_2_to_32_minus_1", [] { Mp m; m.map(1); m.str("item"); m.raw({0xc9, 0xff, 0xff, 0xff, 0xff, 1}); return m.b; }(), "refuse"});
    {
        std::vector<Tensor> unused;
        c.push_back({"record_whose_projection_has_the_bias_that_fc2_lacks", burn_tower(BIN, 1, unused, 1, true), "refuse"});
    }
    c.push_back({"record_without_a_tensor", [] { Mp m; m.map(1); m.str("item"); m.map(1); m.str("abcdef"); m.u(1); return m.b; }(), "refuse"});
    c.push_back({"file_of_8_bytes", le64(2), "refuse"});
    c.push_back({"file_of_9_bytes", le64(1) + "{", "refuse"});
    c.push_back({"empty_file", Bytes(), "refuse"});
    return c;
}

static void hostile(const std::string& dir, const std::string& only) {
    FILE* list = std::fopen((dir + "/hostile.txt").c_str(), "w");
    if (!list) { std::printf("cannot write the list\n"); std::exit(2); }
    for (const Case& c : hostile_cases()) {
        if (c.name.find(only) == std::string::npos) continue;
        const std::string file = "hostile_" + c.name + ".bin", p = dir + "/" + file;
        write_file(p, c.file);
        std::string why;
        const Outcome o = probe(p, c.name, &why);
        const std::string want = c.expect;
        const bool ok = o != WRONG && (want == "any" || (want == "accept") == (o == READ));
        if (!ok) { std::printf("FAILED: %s: want %s, got %s (%s)\n", c.name.c_str(), c.expect, o == READ ? "read" : o == REFUSED ? "refused" : "WRONG", why.c_str()); ++failures; }
        if (o == REFUSED && why.empty()) { std::printf("FAILED: %s: refused without a message\n", c.name.c_str()); ++failures; }
        std::fprintf(list, "%s %s\n", file.c_str(), c.expect);
    }
    std::fclose(list);
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: test_weights_host <scratch dir>\n"); return 2; }
    const std::string dir = argv[1];
    const auto t0 = std::chrono::steady_clock::now();
    const std::string only = argc > 2 ? argv[2] : "";
    if (only.empty()) {
        conversions();
        valid_files(dir);
    }
    hostile(dir, only);
    if (only.empty()) corpus(dir);
    std::printf("slowest file: %s, %.3f s; all of it %.1f s\n", slowest_case.c_str(), slowest,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
