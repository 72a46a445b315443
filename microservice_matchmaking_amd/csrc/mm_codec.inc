// mm_codec.inc — include/mm_codec.h: the enqueue-side codec (host code, included by mm_engine.hip).
// A strict JSON reader (RFC 8259 grammar, UTF-8 checked) that looks at the top-level members the
// search stage reads and skips the rest.

#include "../../include/mm_codec.h"

struct JsonCur {
    const unsigned char* p;
    const unsigned char* end;
};

static inline void js_ws(JsonCur& c)
{
    while (c.p < c.end && (*c.p == ' ' || *c.p == '\t' || *c.p == '\n' || *c.p == '\r')) ++c.p;
}

static inline int js_hex(unsigned char h)
{
    if (h >= '0' && h <= '9') return h - '0';
    if (h >= 'a' && h <= 'f') return h - 'a' + 10;
    if (h >= 'A' && h <= 'F') return h - 'A' + 10;
    return -1;
}

// A string, cursor on the opening quote.  *raw0 / *rawlen: its contents as written.  dec (capacity
// dcap): the contents with escapes resolved, *dlen = their length or dcap + 1 if they did not fit.
static bool js_string(JsonCur& c, const unsigned char** raw0, size_t* rawlen, unsigned char* dec, size_t dcap, size_t* dlen)
{
    if (c.p >= c.end || *c.p != '"') return false;
    ++c.p;
    *raw0 = c.p;
    size_t n = 0;
    auto put = [&](unsigned char b) { if (n < dcap) dec[n] = b; ++n; };
    auto put_cp = [&](uint32_t cp) {
        if (cp < 0x80) put((unsigned char)cp);
        else if (cp < 0x800) { put((unsigned char)(0xC0 | (cp >> 6))); put((unsigned char)(0x80 | (cp & 63))); }
        else if (cp < 0x10000) { put((unsigned char)(0xE0 | (cp >> 12))); put((unsigned char)(0x80 | ((cp >> 6) & 63))); put((unsigned char)(0x80 | (cp & 63))); }
        else { put((unsigned char)(0xF0 | (cp >> 18))); put((unsigned char)(0x80 | ((cp >> 12) & 63))); put((unsigned char)(0x80 | ((cp >> 6) & 63))); put((unsigned char)(0x80 | (cp & 63))); }
    };
    for (;;) {
        if (c.p >= c.end) return false;
        const unsigned char b = *c.p;
        if (b == '"') break;
        if (b < 0x20) return false;
        if (b == '\\') {
            if (c.end - c.p < 2) return false;
            const unsigned char e = c.p[1];
            c.p += 2;
            switch (e) {
            case '"': put('"'); break;
            case '\\': put('\\'); break;
            case '/': put('/'); break;
            case 'b': put('\b'); break;
            case 'f': put('\f'); break;
            case 'n': put('\n'); break;
            case 'r': put('\r'); break;
            case 't': put('\t'); break;
            case 'u': {
                if (c.end - c.p < 4) return false;
                uint32_t cp = 0;
                for (int k = 0; k < 4; ++k) {
                    const int h = js_hex(c.p[k]);
                    if (h < 0) return false;
                    cp = (cp << 4) | (uint32_t)h;
                }
                c.p += 4;
                if (cp >= 0xD800 && cp < 0xDC00 && c.end - c.p >= 6 && c.p[0] == '\\' && c.p[1] == 'u') {
                    uint32_t lo = 0;
                    bool okh = true;
                    for (int k = 0; k < 4; ++k) {
                        const int h = js_hex(c.p[2 + k]);
                        if (h < 0) { okh = false; break; }
                        lo = (lo << 4) | (uint32_t)h;
                    }
                    if (okh && lo >= 0xDC00 && lo < 0xE000) {
                        cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
                        c.p += 6;
                    }
                }
                put_cp(cp);
                break;
            }
            default: return false;
            }
            continue;
        }
        // UTF-8, well formed only (Unicode table 3-7)
        size_t need = 0;
        unsigned char lo = 0x80, hi = 0xBF;
        if (b < 0x80) need = 0;
        else if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b == 0xE0) { need = 2; lo = 0xA0; }
        else if ((b >= 0xE1 && b <= 0xEC) || b == 0xEE || b == 0xEF) need = 2;
        else if (b == 0xED) { need = 2; hi = 0x9F; }
        else if (b == 0xF0) { need = 3; lo = 0x90; }
        else if (b >= 0xF1 && b <= 0xF3) need = 3;
        else if (b == 0xF4) { need = 3; hi = 0x8F; }
        else return false;
        if ((size_t)(c.end - c.p) < need + 1) return false;
        for (size_t k = 1; k <= need; ++k) {
            const unsigned char t = c.p[k];
            if (k == 1 ? (t < lo || t > hi) : (t < 0x80 || t > 0xBF)) return false;
        }
        for (size_t k = 0; k <= need; ++k) put(c.p[k]);
        c.p += need + 1;
    }
    *rawlen = (size_t)(c.p - *raw0);
    ++c.p;                                         // closing quote
    *dlen = n <= dcap ? n : dcap + 1;
    return true;
}

// A number, cursor on its first character.  *is_int: no fraction and no exponent.
static bool js_number(JsonCur& c, const unsigned char** t0, size_t* tlen, bool* is_int)
{
    const unsigned char* s = c.p;
    if (c.p < c.end && *c.p == '-') ++c.p;
    if (c.p >= c.end) return false;
    if (*c.p == '0') ++c.p;
    else if (*c.p >= '1' && *c.p <= '9') { while (c.p < c.end && *c.p >= '0' && *c.p <= '9') ++c.p; }
    else return false;
    *is_int = true;
    if (c.p < c.end && *c.p == '.') {
        ++c.p;
        if (c.p >= c.end || *c.p < '0' || *c.p > '9') return false;
        while (c.p < c.end && *c.p >= '0' && *c.p <= '9') ++c.p;
        *is_int = false;
    }
    if (c.p < c.end && (*c.p == 'e' || *c.p == 'E')) {
        ++c.p;
        if (c.p < c.end && (*c.p == '+' || *c.p == '-')) ++c.p;
        if (c.p >= c.end || *c.p < '0' || *c.p > '9') return false;
        while (c.p < c.end && *c.p >= '0' && *c.p <= '9') ++c.p;
        *is_int = false;
    }
    *t0 = s;
    *tlen = (size_t)(c.p - s);
    return true;
}

static bool js_literal(JsonCur& c, const char* w)
{
    const size_t n = strlen(w);
    if ((size_t)(c.end - c.p) < n || memcmp(c.p, w, n) != 0) return false;
    c.p += n;
    return true;
}

// Any value: checked and skipped.
static bool js_skip(JsonCur& c, int depth)
{
    if (depth > 512) return false;          // deliberate limit (documented in mm_codec.h)
    js_ws(c);
    if (c.p >= c.end) return false;
    const unsigned char b = *c.p;
    if (b == '"') {
        const unsigned char* r0;
        size_t rl, dl;
        return js_string(c, &r0, &rl, NULL, 0, &dl);
    }
    if (b == '{') {
        ++c.p;
        js_ws(c);
        if (c.p < c.end && *c.p == '}') { ++c.p; return true; }
        for (;;) {
            js_ws(c);
            const unsigned char* r0;
            size_t rl, dl;
            if (!js_string(c, &r0, &rl, NULL, 0, &dl)) return false;
            js_ws(c);
            if (c.p >= c.end || *c.p != ':') return false;
            ++c.p;
            if (!js_skip(c, depth + 1)) return false;
            js_ws(c);
            if (c.p >= c.end) return false;
            if (*c.p == ',') { ++c.p; continue; }
            if (*c.p == '}') { ++c.p; return true; }
            return false;
        }
    }
    if (b == '[') {
        ++c.p;
        js_ws(c);
        if (c.p < c.end && *c.p == ']') { ++c.p; return true; }
        for (;;) {
            if (!js_skip(c, depth + 1)) return false;
            js_ws(c);
            if (c.p >= c.end) return false;
            if (*c.p == ',') { ++c.p; continue; }
            if (*c.p == ']') { ++c.p; return true; }
            return false;
        }
    }
    if (b == 't') return js_literal(c, "true");
    if (b == 'f') return js_literal(c, "false");
    if (b == 'n') return js_literal(c, "null");
    const unsigned char* t0;
    size_t tl;
    bool ii;
    return js_number(c, &t0, &tl, &ii);
}

struct DecField {            // one member the codec looks at
    int kind;                // 0 absent, 1 number, 2 string, 3 anything else
    bool is_int;
    const unsigned char* t0; // number text / string contents as written
    size_t tlen;
    unsigned char dec[72];   // string with escapes resolved
    size_t dlen;
};

static bool dec_key_is(const unsigned char* k, size_t klen, const char* name)
{
    return name && strlen(name) == klen && memcmp(k, name, klen) == 0;
}

// number text -> value.  *exact32: an integer that fits int32 (integral floats included).
static double dec_number(const DecField& f, bool* exact32, int32_t* as_i32)
{
    char tmp[80];
    double v;
    if (f.tlen < sizeof(tmp)) {
        memcpy(tmp, f.t0, f.tlen);
        tmp[f.tlen] = 0;
        v = strtod(tmp, NULL);
    } else {
        std::vector<char> big(f.t0, f.t0 + f.tlen);
        big.push_back(0);
        v = strtod(big.data(), NULL);
    }
    *exact32 = false;
    if (v >= -2147483648.0 && v <= 2147483647.0) {
        const double fl = v < 0 ? -(double)(long long)(-v) : (double)(long long)v;   // trunc
        if (fl == v) { *exact32 = true; *as_i32 = (int32_t)v; return v; }
        const double flo = v < fl ? fl - 1.0 : fl;                                   // floor
        *as_i32 = (int32_t)flo;
    } else *as_i32 = v < 0 ? (int32_t)0x80000000 : 0x7FFFFFFF;
    return v;
}

static int decode_players_impl(const mm_config* cfg, const mm_codec_cfg* cc, const char* buf, const uint64_t* off, uint32_t n,
                               int32_t* rating, uint32_t* cons, uint8_t* group, uint8_t* status,
                               uint32_t* id_off, uint32_t* id_len);

extern "C" int mm_decode_players(const mm_config* cfg, const mm_codec_cfg* cc, const char* buf, const uint64_t* off, uint32_t n,
                                 int32_t* rating, uint32_t* cons, uint8_t* group, uint8_t* status,
                                 uint32_t* id_off, uint32_t* id_len)
{
    return guarded([&]() -> int {                      // nothing unwinds into a NIF frame
        return decode_players_impl(cfg, cc, buf, off, n, rating, cons, group, status, id_off, id_len);
    });
}

static int decode_players_impl(const mm_config* cfg, const mm_codec_cfg* cc, const char* buf, const uint64_t* off, uint32_t n,
                               int32_t* rating, uint32_t* cons, uint8_t* group, uint8_t* status,
                               uint32_t* id_off, uint32_t* id_len)
{
    if (!cfg || !cc || (n && (!buf || !off || !rating || !cons || !group || !status))) return MM_ERR_INVALID_ARG;
    if (cc->n_modes > cfg->n_modes || cfg->default_group >= cfg->n_groups) return MM_ERR_INVALID_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return MM_ERR_INVALID_ARG;
        rating[i] = 0;
        cons[i] = 0;
        group[i] = 0;
        if (id_off) id_off[i] = 0;
        if (id_len) id_len[i] = 0;
        const unsigned char* const m0 = (const unsigned char*)buf + off[i];
        JsonCur c{m0, (const unsigned char*)buf + off[i + 1]};
        DecField f_rating{}, f_mode{}, f_id{}, f_region{}, f_party{}, f_role{};
        bool ok = true;
        js_ws(c);
        if (c.p >= c.end || *c.p != '{') ok = false;
        else {
            ++c.p;
            js_ws(c);
            if (c.p < c.end && *c.p == '}') ++c.p;
            else
                for (;;) {
                    js_ws(c);
                    unsigned char key[72];
                    const unsigned char* r0;
                    size_t rl, kl;
                    if (!js_string(c, &r0, &rl, key, sizeof(key), &kl)) { ok = false; break; }
                    js_ws(c);
                    if (c.p >= c.end || *c.p != ':') { ok = false; break; }
                    ++c.p;
                    js_ws(c);
                    DecField* f = NULL;
                    if (kl <= sizeof(key)) {
                        if (dec_key_is(key, kl, "rating")) f = &f_rating;
                        else if (dec_key_is(key, kl, "game-mode")) f = &f_mode;
                        else if (dec_key_is(key, kl, "id")) f = &f_id;
                        else if (dec_key_is(key, kl, cc->region_key)) f = &f_region;
                        else if (dec_key_is(key, kl, cc->party_key)) f = &f_party;
                        else if (dec_key_is(key, kl, cc->role_key)) f = &f_role;
                    }
                    if (!f) {
                        if (!js_skip(c, 1)) { ok = false; break; }
                    } else if (c.p < c.end && *c.p == '"') {
                        f->kind = 2;
                        if (!js_string(c, &f->t0, &f->tlen, f->dec, sizeof(f->dec), &f->dlen)) { ok = false; break; }
                    } else if (c.p < c.end && (*c.p == '-' || (*c.p >= '0' && *c.p <= '9'))) {
                        f->kind = 1;
                        if (!js_number(c, &f->t0, &f->tlen, &f->is_int)) { ok = false; break; }
                    } else {
                        f->kind = 3;
                        if (!js_skip(c, 1)) { ok = false; break; }
                    }
                    js_ws(c);
                    if (c.p >= c.end) { ok = false; break; }
                    if (*c.p == ',') { ++c.p; continue; }
                    if (*c.p == '}') { ++c.p; break; }
                    ok = false;
                    break;
                }
            if (ok) {
                js_ws(c);
                if (c.p != c.end) ok = false;      // something behind the object
            }
        }
        if (!ok) { status[i] = (uint8_t)MM_DEC_BAD_JSON; continue; }
        // "game-mode" (worker.ex:294)
        uint32_t mode = cc->n_modes;
        if (f_mode.kind == 2 && f_mode.dlen <= sizeof(f_mode.dec))
            for (uint32_t k = 0; k < cc->n_modes; ++k)
                if (dec_key_is(f_mode.dec, f_mode.dlen, cc->mode_name[k])) { mode = k; break; }
        if (mode >= cc->n_modes) { status[i] = (uint8_t)MM_DEC_NO_MODE; continue; }
        // extension fields
        uint32_t ext[3] = {0, 0, 0};
        const DecField* ef[3] = {&f_region, &f_party, &f_role};
        const uint32_t emax[3] = {255u, 15u, 15u};
        bool ext_ok = true;
        for (int k = 0; k < 3; ++k) {
            if (ef[k]->kind == 0) continue;
            bool e32 = false;
            int32_t v32 = 0;
            if (ef[k]->kind != 1 || !ef[k]->is_int) { ext_ok = false; break; }
            dec_number(*ef[k], &e32, &v32);
            if (!e32 || v32 < 0 || (uint32_t)v32 > emax[k]) { ext_ok = false; break; }
            ext[k] = (uint32_t)v32;
        }
        if (!ext_ok) { status[i] = (uint8_t)MM_DEC_BAD_FIELD; continue; }
        cons[i] = MM_CONS_MAKE(mode, ext[0], ext[1], ext[2]);
        if (f_id.kind == 1 || f_id.kind == 2) {
            if (id_off) id_off[i] = (uint32_t)(f_id.t0 - m0);
            if (id_len) id_len[i] = (uint32_t)f_id.tlen;
        }
        // "rating" (generic/worker.ex:57) and its group (:46-53)
        if (f_rating.kind == 1) {
            bool e32 = false;
            int32_t v32 = 0;
            const double v = dec_number(f_rating, &e32, &v32);
            uint32_t g = cfg->default_group;
            (void)mm_find_rating_group(cfg, v, &g);
            rating[i] = v32;
            group[i] = (uint8_t)g;
            status[i] = (uint8_t)(e32 ? MM_DEC_OK : MM_DEC_RATING_INEXACT);
        } else {
            group[i] = (uint8_t)cfg->default_group;
            status[i] = (uint8_t)MM_DEC_RATING_NOT_NUMBER;
        }
    }
    return MM_OK;
}

// ------------------------------------------------------------------------------------
// mm_encode_lobby: the bytes Poison 4.0.1 (mix.lock:17) writes for
//   Poison.encode!(%{"teams" => updated_grouped_players, "game-mode" => game_mode})   worker.ex:315-318
// where every player is the map Poison.decode! made of its delivery, minus "game-mode" (worker.ex:292-294).
// Poison decodes and re-encodes, so every value is re-written in Poison's canonical form:
//   map     Poison.Encoder.Map: `:lists.foldl(fun, [], :maps.keys(map))` with `fun` PREPENDING each member
//           -> members in the REVERSE of :maps.keys/1.  For a map of <= 32 keys (a flatmap) :maps.keys/1 is
//           ascending term order = bytewise order of the (binary) keys, so the output is in DESCENDING key
//           order ({"teams":..,"game-mode":..}; "team 2" before "team 1").  A duplicate member keeps its
//           last value (Map.put while decoding).  Beyond 32 keys the VM's hash order applies, which cannot
//           be restated here: such an object is still written in descending order and is only map-equal.
//   list    Poison.Encoder.List: `:lists.foldr` — order kept.
//   string  Poison.Encoder.BitString, default escape mode: \" \\ \n \t \r \f \b, every other byte <= 0x1F and
//           0x7F as \u00XX with UPPERCASE hex digits (Integer.to_charlist(c, 16)), everything else — "/" and
//           all of UTF-8 included — as is.  Escapes of the input (A, \/) are resolved first.
//   integer Integer.to_string of the decoded value: the digits as written ("-0" is 0).
//   float   :io_lib_format.fwrite_g/1: the shortest digits that read back to the same double, laid out by
//           insert_decimal/2 (fixed notation unless the exponent form is strictly shorter: 100.0, 1.0e3,
//           0.001, 1.0e-5, 2500.5).  A number with a fraction or an exponent is a float to Poison (1e3 -> 1.0e3).
//   true / false / null as written.
// Derived from the Poison 4.0.1 / OTP sources as restated above; no BEAM is available in this image to run
// them (SURVEY.md F8), so tests/test_codec.py pins these rules with hand-derived golden strings and an
// independent Python restatement, and still checks map equality with Python's json.
// ------------------------------------------------------------------------------------
struct EncMember {
    std::vector<unsigned char> key;      // escapes resolved
    const unsigned char* v0;             // the value as written
    size_t vlen;
};

struct EncOut {
    char* p;
    uint64_t cap, n;
    void put(const void* b, size_t len)
    {
        if (n + len <= cap) memcpy(p + n, b, len);
        n += len;
    }
    void ch(char c) { put(&c, 1); }
    void str(const unsigned char* b, size_t len)     // Poison.Encoder.BitString, default escape mode
    {
        ch('"');
        size_t run = 0;                              // bytes copied as they are, flushed in one piece
        for (size_t i = 0; i < len; ++i) {
            const unsigned char c = b[i];
            const char* esc = NULL;
            char u[8];
            switch (c) {
            case '"': esc = "\\\""; break;
            case '\\': esc = "\\\\"; break;
            case '\n': esc = "\\n"; break;
            case '\t': esc = "\\t"; break;
            case '\r': esc = "\\r"; break;
            case '\f': esc = "\\f"; break;
            case '\b': esc = "\\b"; break;
            default:
                if (c <= 0x1F || c == 0x7F) {
                    snprintf(u, sizeof(u), "\\u%04X", (unsigned)c);
                    esc = u;
                }
            }
            if (!esc) { ++run; continue; }
            if (run) put(b + i - run, run);
            run = 0;
            put(esc, strlen(esc));
        }
        if (run) put(b + len - run, run);
        ch('"');
    }
};

// :io_lib_format.fwrite_g/1 for a finite double
static void enc_float(double v, EncOut& o)
{
    // Both zeros print "0.0": the reference runs on the elixir:1.6.2 image (OTP 20), where -0.0 =:= 0.0 and the
    // `fwrite_g(0.0)` clause of io_lib_format takes negative zero too (the zeros only became distinct terms in OTP 27).
    if (v == 0.0) { o.put("0.0", 3); return; }
    const double a = v < 0 ? -v : v;
    char buf[48];
    int prec = 1;
    for (; prec <= 17; ++prec) {                      // shortest digit string that reads back exactly
        snprintf(buf, sizeof(buf), "%.*e", prec - 1, a);
        if (strtod(buf, NULL) == a) break;
    }
    char digits[24];
    int L = 0;
    const char* q = buf;
    for (; *q && *q != 'e'; ++q)
        if (*q >= '0' && *q <= '9') digits[L++] = *q;
    const int place = atoi(q + 1) + 1;                // value = 0.DIGITS * 10^place
    if (v < 0) o.ch('-');
    char expl[16];
    const int expn = snprintf(expl, sizeof(expl), "%d", place - 1);
    auto with_exp = [&]() {                           // insert_exp/2
        o.put(digits, 1);
        o.ch('.');
        if (L == 1) o.ch('0');
        else o.put(digits + 1, (size_t)L - 1);
        o.ch('e');
        o.put(expl, (size_t)expn);
    };
    if (place == 0) { o.put("0.", 2); o.put(digits, (size_t)L); return; }
    if (place < 0 || place >= L) {
        const int exp_cost = expn + 1 + (L == 1 ? 2 : 1);
        if (place < 0) {
            if (2 - place <= exp_cost) {
                o.put("0.", 2);
                for (int k = 0; k < -place; ++k) o.ch('0');
                o.put(digits, (size_t)L);
            } else with_exp();
        } else {
            if (place - L + 2 <= exp_cost) {
                o.put(digits, (size_t)L);
                for (int k = 0; k < place - L; ++k) o.ch('0');
                o.put(".0", 2);
            } else with_exp();
        }
        return;
    }
    o.put(digits, (size_t)place);
    o.ch('.');
    o.put(digits + place, (size_t)(L - place));
}

static bool enc_value(JsonCur& c, EncOut& o, int depth, bool drop_game_mode);

// the members of one object in Poison's order (descending keys), last duplicate wins
static bool enc_object(JsonCur& c, EncOut& o, int depth, bool drop_game_mode)
{
    std::vector<EncMember> mem;
    ++c.p;                                            // '{'
    js_ws(c);
    if (c.p < c.end && *c.p == '}') ++c.p;
    else
        for (;;) {
            js_ws(c);
            // key: resolve the escapes (names longer than the scratch are measured first)
            JsonCur k0 = c;
            const unsigned char* r0;
            size_t rl, dl;
            unsigned char small[64];
            if (!js_string(c, &r0, &rl, small, sizeof(small), &dl)) return false;
            EncMember m;
            if (dl <= sizeof(small)) m.key.assign(small, small + dl);
            else {
                m.key.resize(rl);                     // resolved length <= written length
                JsonCur k1 = k0;
                size_t dl2;
                if (!js_string(k1, &r0, &rl, m.key.data(), m.key.size(), &dl2) || dl2 > m.key.size()) return false;
                m.key.resize(dl2);
            }
            js_ws(c);
            if (c.p >= c.end || *c.p != ':') return false;
            ++c.p;
            js_ws(c);
            m.v0 = c.p;
            if (!js_skip(c, depth + 1)) return false;
            m.vlen = (size_t)(c.p - m.v0);
            const bool is_mode = drop_game_mode && m.key.size() == 9 && memcmp(m.key.data(), "game-mode", 9) == 0;
            if (!is_mode) {
                bool dup = false;
                for (EncMember& x : mem)
                    if (x.key == m.key) { x.v0 = m.v0; x.vlen = m.vlen; dup = true; break; }
                if (!dup) mem.push_back(std::move(m));
            }
            js_ws(c);
            if (c.p >= c.end) return false;
            if (*c.p == ',') { ++c.p; continue; }
            if (*c.p == '}') { ++c.p; break; }
            return false;
        }
    std::sort(mem.begin(), mem.end(), [](const EncMember& x, const EncMember& y) { return y.key < x.key; });
    o.ch('{');
    for (size_t j = 0; j < mem.size(); ++j) {
        if (j) o.ch(',');
        o.str(mem[j].key.data(), mem[j].key.size());
        o.ch(':');
        JsonCur v{mem[j].v0, mem[j].v0 + mem[j].vlen};
        if (!enc_value(v, o, depth + 1, false)) return false;
    }
    o.ch('}');
    return true;
}

// one value, checked and re-written in Poison's canonical form; the cursor ends behind it
static bool enc_value(JsonCur& c, EncOut& o, int depth, bool drop_game_mode)
{
    if (depth > 512) return false;
    js_ws(c);
    if (c.p >= c.end) return false;
    const unsigned char b = *c.p;
    if (b == '{') return enc_object(c, o, depth, drop_game_mode);
    if (b == '[') {
        ++c.p;
        o.ch('[');
        js_ws(c);
        if (c.p < c.end && *c.p == ']') { ++c.p; o.ch(']'); return true; }
        for (bool first = true;; first = false) {
            if (!first) o.ch(',');
            if (!enc_value(c, o, depth + 1, false)) return false;
            js_ws(c);
            if (c.p >= c.end) return false;
            if (*c.p == ',') { ++c.p; continue; }
            if (*c.p == ']') { ++c.p; o.ch(']'); return true; }
            return false;
        }
    }
    if (b == '"') {
        JsonCur k0 = c;
        const unsigned char* r0;
        size_t rl, dl;
        unsigned char small[128];
        if (!js_string(c, &r0, &rl, small, sizeof(small), &dl)) return false;
        if (dl <= sizeof(small)) { o.str(small, dl); return true; }
        std::vector<unsigned char> big(rl);           // resolved length <= written length
        size_t dl2;
        if (!js_string(k0, &r0, &rl, big.data(), big.size(), &dl2) || dl2 > big.size()) return false;
        o.str(big.data(), dl2);
        return true;
    }
    if (b == 't') { if (!js_literal(c, "true")) return false; o.put("true", 4); return true; }
    if (b == 'f') { if (!js_literal(c, "false")) return false; o.put("false", 5); return true; }
    if (b == 'n') { if (!js_literal(c, "null")) return false; o.put("null", 4); return true; }
    const unsigned char* t0;
    size_t tl;
    bool is_int;
    if (!js_number(c, &t0, &tl, &is_int)) return false;
    if (is_int) {
        if (tl == 2 && t0[0] == '-' && t0[1] == '0') o.ch('0');       // String.to_integer("-0") = 0
        else o.put(t0, tl);
        return true;
    }
    std::vector<char> txt(t0, t0 + tl);
    txt.push_back(0);
    const double v = strtod(txt.data(), NULL);
    if (!(v - v == 0.0)) return false;                // beyond the doubles: Poison raises on it
    enc_float(v, o);
    return true;
}

extern "C" int mm_encode_lobby(const char* game_mode, uint32_t teams, uint32_t team_size, const char* const* payload,
                               const uint32_t* payload_len, char* out, uint64_t cap, uint64_t* written)
{
    if (!game_mode || !payload || !payload_len || !written || (cap && !out)) return MM_ERR_INVALID_ARG;
    if (teams < 1 || teams > MM_MAX_TEAMS || team_size < 1 || teams * team_size > MM_MAX_LOBBY) return MM_ERR_INVALID_ARG;
    return guarded([&]() -> int {
        EncOut o{out, cap, 0};
        // descending keys on every level: "teams" > "game-mode"; "team 2" > "team 1" (fewer than ten teams)
        o.put("{\"teams\":{", 10);
        for (uint32_t t = teams; t-- > 0;) {
            if (t + 1u != teams) o.ch(',');
            char name[16];
            const int nl = snprintf(name, sizeof(name), "team %u", t + 1u);
            o.str((const unsigned char*)name, (size_t)nl);
            o.put(":[", 2);
            for (uint32_t k = 0; k < team_size; ++k) {
                const uint32_t i = t * team_size + k;
                if (!payload[i]) return MM_ERR_INVALID_ARG;
                if (k) o.ch(',');
                JsonCur c{(const unsigned char*)payload[i], (const unsigned char*)payload[i] + payload_len[i]};
                js_ws(c);
                if (c.p >= c.end || *c.p != '{' || !enc_object(c, o, 0, true)) return MM_ERR_INVALID_ARG;
                js_ws(c);
                if (c.p != c.end) return MM_ERR_INVALID_ARG;          // something behind the object
            }
            o.ch(']');
        }
        o.put("},\"game-mode\":", 14);
        o.str((const unsigned char*)game_mode, strlen(game_mode));
        o.ch('}');
        *written = o.n;
        return o.n <= cap ? MM_OK : MM_ERR_RANGE;
    });
}
