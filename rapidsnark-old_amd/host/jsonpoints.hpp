// Reading snarkjs's JSON files, what `verifier` (Groth16) and `plonkverifier` share: a file as a string, a decimal integer,
// a point of G1 or G2 as an array of coordinates, a member of an object.  Points are decimal strings (or bare numbers); a
// third projective coordinate is honoured: 0 is the point at infinity, anything else divides x and y.
#pragma once
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>

#include "../csrc/curve.hpp"
#include "json_min.hpp"
#include "zkfile.hpp"

namespace JsonPoints {

using JsonMin::Value;
using zk::Fq;
using zk::Fq2;

inline std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::invalid_argument(path + ": cannot be opened");
    std::ostringstream o;
    o << f.rdbuf();
    return o.str();
}

// a decimal integer below 2^256, as a JSON string or a bare number -> 32 little-endian bytes
inline void decimal(const Value &v, const std::string &what, void *out) {
    if ((v.type != Value::String && v.type != Value::Number) || !U256::from_dec(v.text, static_cast<uint8_t *>(out)))
        throw std::invalid_argument(what + " is not a decimal integer below 2^256");
}
inline bool below_q(const void *le) { return U256::less(static_cast<const uint8_t *>(le), U256::kBn254Q.data()); }
// The coordinate as the library takes it: Montgomery form.  One that is not below q is passed as written, so that the
// device's own check refuses the proof (`reduced` tells the caller that nothing may be computed with it here).
inline Fq coord(const Value &v, const std::string &what, bool &reduced) {
    Fq x;
    decimal(v, what, x.v);
    if (!below_q(x.v)) {
        reduced = false;
        return x;
    }
    return Fq::to_mont(x);
}
inline const Value &item(const Value &v, size_t i, const std::string &what) {
    if (v.type != Value::Array || v.items.size() <= i) throw std::invalid_argument(what + " is not an array of at least " + std::to_string(i + 1) + " elements");
    return v.items[i];
}

inline void g1_point(const Value &v, const std::string &what, uint8_t out[64]) {
    bool red = true;
    Fq x = coord(item(v, 0, what), what + "[0]", red), y = coord(item(v, 1, what), what + "[1]", red);
    if (v.items.size() > 2) {
        const Fq z = coord(v.items[2], what + "[2]", red);
        if (red && z.is_zero()) {
            memset(out, 0, 64);
            return;
        }
        if (red && z != Fq::one()) {
            const Fq zi = Fq::inv(z);
            x = Fq::mul(x, zi);
            y = Fq::mul(y, zi);
        }
    }
    memcpy(out, x.v, 32);
    memcpy(out + 32, y.v, 32);
}
inline void g2_point(const Value &v, const std::string &what, uint8_t out[128]) {
    bool red = true;
    auto f2 = [&](size_t i) {
        const std::string w = what + "[" + std::to_string(i) + "]";
        const Value &c = item(v, i, what);
        Fq2 r;
        r.a = coord(item(c, 0, w), w + "[0]", red);
        r.b = coord(item(c, 1, w), w + "[1]", red);
        return r;
    };
    Fq2 x = f2(0), y = f2(1);
    if (v.items.size() > 2) {
        const Fq2 z = f2(2);
        if (red && z.is_zero()) {
            memset(out, 0, 128);
            return;
        }
        if (red && z != Fq2::one()) {
            const Fq2 zi = Fq2::inv(z);
            x = Fq2::mul(x, zi);
            y = Fq2::mul(y, zi);
        }
    }
    memcpy(out, x.a.v, 32);
    memcpy(out + 32, x.b.v, 32);
    memcpy(out + 64, y.a.v, 32);
    memcpy(out + 96, y.b.v, 32);
}
inline const Value &member(const Value &o, const char *key, const std::string &file) {
    const Value *m = o.type == Value::Object ? o.find(key) : nullptr;
    if (!m) throw std::invalid_argument(file + ": no \"" + key + "\"");
    return *m;
}

inline Value parse_file(const std::string &path) {
    try {
        return JsonMin::parse(slurp(path));
    } catch (const std::invalid_argument &e) {
        const std::string m = e.what();
        throw std::invalid_argument(m.compare(0, 5, "JSON:") == 0 ? path + ": " + m : m);
    }
}

}   // namespace JsonPoints
