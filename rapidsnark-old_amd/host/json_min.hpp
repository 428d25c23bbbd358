// Minimal JSON helpers for the server shell: syntax validation of a request body and string
// escaping for the status document.  (The reference links nlohmann/json, an empty submodule in
// its checkout; the only JSON produced here are the fixed shapes of SURVEY §A.3.)
#pragma once
#include <cctype>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace JsonMin {

class Validator {
    const std::string &s;
    size_t p = 0;
    int depth = 0;
    void ws() { while (p < s.size() && (s[p] == ' ' || s[p] == '\t' || s[p] == '\n' || s[p] == '\r')) p++; }
    bool lit(const char *w) {
        size_t n = 0;
        while (w[n]) n++;
        if (s.compare(p, n, w) != 0) return false;
        p += n;
        return true;
    }
    bool str() {
        if (p >= s.size() || s[p] != '"') return false;
        p++;
        while (p < s.size()) {
            unsigned char c = (unsigned char)s[p++];
            if (c == '"') return true;
            if (c < 0x20) return false;
            if (c == '\\') {
                if (p >= s.size()) return false;
                char e = s[p++];
                if (e == 'u') {
                    for (int i = 0; i < 4; i++)
                        if (p >= s.size() || !isxdigit((unsigned char)s[p++])) return false;
                } else if (!(e == '"' || e == '\\' || e == '/' || e == 'b' || e == 'f' || e == 'n' || e == 'r' || e == 't'))
                    return false;
            }
        }
        return false;
    }
    bool num() {
        size_t st = p;
        if (p < s.size() && s[p] == '-') p++;
        if (p >= s.size()) return false;
        if (s[p] == '0') p++;
        else if (isdigit((unsigned char)s[p])) while (p < s.size() && isdigit((unsigned char)s[p])) p++;
        else return false;
        if (p < s.size() && s[p] == '.') {
            p++;
            if (p >= s.size() || !isdigit((unsigned char)s[p])) return false;
            while (p < s.size() && isdigit((unsigned char)s[p])) p++;
        }
        if (p < s.size() && (s[p] == 'e' || s[p] == 'E')) {
            p++;
            if (p < s.size() && (s[p] == '+' || s[p] == '-')) p++;
            if (p >= s.size() || !isdigit((unsigned char)s[p])) return false;
            while (p < s.size() && isdigit((unsigned char)s[p])) p++;
        }
        return p > st;
    }
    bool value() {
        if (++depth > 512) return false;
        ws();
        bool ok = false;
        if (p >= s.size()) ok = false;
        else if (s[p] == '{') {
            p++;
            ws();
            if (p < s.size() && s[p] == '}') { p++; ok = true; }
            else
                for (;;) {
                    ws();
                    if (!str()) break;
                    ws();
                    if (p >= s.size() || s[p++] != ':') break;
                    if (!value()) break;
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == '}') { p++; ok = true; }
                    break;
                }
        } else if (s[p] == '[') {
            p++;
            ws();
            if (p < s.size() && s[p] == ']') { p++; ok = true; }
            else
                for (;;) {
                    if (!value()) break;
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == ']') { p++; ok = true; }
                    break;
                }
        } else if (s[p] == '"') ok = str();
        else if (s[p] == 't') ok = lit("true");
        else if (s[p] == 'f') ok = lit("false");
        else if (s[p] == 'n') ok = lit("null");
        else ok = num();
        depth--;
        return ok;
    }

public:
    explicit Validator(const std::string &text) : s(text) {}
    bool valid() {
        if (!value()) return false;
        ws();
        return p == s.size();
    }
};

inline bool isValid(const std::string &text) { return Validator(text).valid(); }

// "..." with the escapes nlohmann's dump() emits for these characters
inline std::string quote(const std::string &v) {
    std::string o = "\"";
    for (unsigned char c : v) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            default:
                if (c < 0x20) {
                    char buf[8];
                    snprintf(buf, sizeof buf, "\\u%04x", c);
                    o += buf;
                } else
                    o += (char)c;
        }
    }
    return o + "\"";
}

// A parsed document, for the few JSON files the tools READ (verifier: proof.json, public.json, verification_key.json).
// Numbers keep their text (the values of interest are 254-bit integers, written as strings or as bare numbers); strings
// are unescaped except \u sequences, which none of these files use in a value that is looked at.
struct Value {
    enum Type { Null, Bool, Number, String, Array, Object } type = Null;
    std::string text;                                  // Number: as written; String: the content; Bool: "true" / "false"
    std::vector<Value> items;                          // Array
    std::vector<std::pair<std::string, Value>> members;   // Object, in file order
    const Value *find(const std::string &key) const {
        for (const auto &m : members)
            if (m.first == key) return &m.second;
        return nullptr;
    }
};

class Parser {
    const std::string &s;
    size_t p = 0;
    int depth = 0;
    [[noreturn]] void fail(const char *what) const { throw std::invalid_argument(std::string("JSON: ") + what + " at byte " + std::to_string(p)); }
    void ws() { while (p < s.size() && (s[p] == ' ' || s[p] == '\t' || s[p] == '\n' || s[p] == '\r')) p++; }
    std::string str() {
        std::string o;
        p++;                                           // the opening quote
        for (;;) {
            if (p >= s.size()) fail("unterminated string");
            const unsigned char c = (unsigned char)s[p++];
            if (c == '"') return o;
            if (c < 0x20) fail("control character in a string");
            if (c != '\\') {
                o += (char)c;
                continue;
            }
            if (p >= s.size()) fail("unterminated string");
            const char e = s[p++];
            switch (e) {
                case '"': case '\\': case '/': o += e; break;
                case 'b': o += '\b'; break;
                case 'f': o += '\f'; break;
                case 'n': o += '\n'; break;
                case 'r': o += '\r'; break;
                case 't': o += '\t'; break;
                case 'u':
                    for (int i = 0; i < 4; i++)
                        if (p >= s.size() || !isxdigit((unsigned char)s[p++])) fail("bad \\u escape");
                    o += '?';
                    break;
                default: fail("bad escape");
            }
        }
    }
    Value value() {
        if (++depth > 512) fail("nesting too deep");
        ws();
        Value v;
        if (p >= s.size()) fail("value expected");
        const char c = s[p];
        if (c == '{') {
            v.type = Value::Object;
            p++;
            ws();
            if (p < s.size() && s[p] == '}') p++;
            else
                for (;;) {
                    ws();
                    if (p >= s.size() || s[p] != '"') fail("member name expected");
                    std::string key = str();
                    ws();
                    if (p >= s.size() || s[p++] != ':') fail("':' expected");
                    v.members.emplace_back(std::move(key), value());
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == '}') { p++; break; }
                    fail("',' or '}' expected");
                }
        } else if (c == '[') {
            v.type = Value::Array;
            p++;
            ws();
            if (p < s.size() && s[p] == ']') p++;
            else
                for (;;) {
                    v.items.push_back(value());
                    ws();
                    if (p < s.size() && s[p] == ',') { p++; continue; }
                    if (p < s.size() && s[p] == ']') { p++; break; }
                    fail("',' or ']' expected");
                }
        } else if (c == '"') {
            v.type = Value::String;
            v.text = str();
        } else if (s.compare(p, 4, "true") == 0) {
            v.type = Value::Bool; v.text = "true"; p += 4;
        } else if (s.compare(p, 5, "false") == 0) {
            v.type = Value::Bool; v.text = "false"; p += 5;
        } else if (s.compare(p, 4, "null") == 0) {
            p += 4;
        } else {
            const size_t st = p;
            while (p < s.size() && (isdigit((unsigned char)s[p]) || s[p] == '-' || s[p] == '+' || s[p] == '.' || s[p] == 'e' || s[p] == 'E')) p++;
            if (p == st || !isValid(s.substr(st, p - st))) { p = st; fail("value expected"); }
            v.type = Value::Number;
            v.text = s.substr(st, p - st);
        }
        depth--;
        return v;
    }

public:
    explicit Parser(const std::string &text) : s(text) {}
    Value parse() {
        Value v = value();
        ws();
        if (p != s.size()) fail("text after the document");
        return v;
    }
};

// throws std::invalid_argument("JSON: ... at byte N") for text that is not one JSON document
inline Value parse(const std::string &text) { return Parser(text).parse(); }

}   // namespace JsonMin
