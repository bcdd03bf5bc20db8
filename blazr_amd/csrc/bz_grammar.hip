// bz_grammar.hip -- grammar-constrained decoding: GBNF -> DFA on the host, the logit mask on the device.
//   parse_gbnf / parse_gbnf_sequence        /root/reference/src/engine/grammar_parser.rs:47-190
//   GrammarDfa                              /root/reference/src/engine/grammar.rs:21-64
//   compute_token_mask / to_device          /root/reference/src/engine/grammar.rs:69-84, 90-139
//   mask_logits                             /root/reference/src/engine/grammar.rs:142-158
//   compile_grammar_to_dfa                  /root/reference/src/engine/grammar.rs:165-277
//   GrammarDfaOps::grammar_dfa_mask_logits  /root/reference/src/engine/sampling.rs:415-419 (the trait and its kernel live in the absent boostr)
//
// flags == 0 restates the reference's compiler statement by statement, quirks included: a line is split at its first "::=", a body at EVERY '|'
// (before quotes are looked at), '#' lines are comments, the escape table is \n \t \" \\ (anything else keeps its backslash), a class member is
// `ch as u8` (the code point truncated to its low byte), only the first rule named `root` is expanded, a literal is a chain of byte states, a class is
// one state, and EVERY OTHER ELEMENT (rule reference, negated class, name* name+ name?) is one state reached by any byte 0..=127.  No `root`
// rule gives a one-state DFA without transitions.
// Three places where the restatement cannot be literal:
//   (a) the reference numbers the DFA states in HashMap iteration order, i.e. arbitrarily.  Here the subset construction visits the bytes in
//       ascending order, so the numbering is canonical (breadth first, ascending byte): equality with the reference is equality of the language and
//       of prefix viability, not of state ids.
//   (b) parse_gbnf_sequence never consumes a character that is neither '"', '[', blank nor a name character (grammar_parser.rs:153-185: empty
//       `name`, no chars.next()), so '(' , ')' or a '*' '+' '?' after a literal or a class spins forever there.  Here that is BZ_E_UNSUPPORTED
//       naming line and column; every loop below consumes at least one character per iteration.
//   (c) the reference's name test is char::is_alphanumeric over all of Unicode.  That table is not carried: a non-ASCII character outside quotes
//       and brackets is BZ_E_UNSUPPORTED as well (inside them it is handled as the reference does: UTF-8 bytes in a literal, `as u8` in a class).
// flags == BZ_GRAMMAR_REGULAR is beyond the reference: the regular subset of GBNF compiled properly (Thompson NFA with epsilon moves, subset
// construction, the same canonical numbering, transitions into states that cannot reach an accepting state removed so that "no byte rejected"
// means "some accepted string extends this prefix").
//
// Device side: the value of boostr's INVALID_STATE is not visible (grammar.rs:9 imports it); here the table is uint16_t with 0xFFFF = none.
// Which rows boostr's kernel masks is not visible either; here the LAST row (the only row logits_to_token reads) is masked and the others are copied.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <bitset>
#include <map>
#include <string>
#include <vector>

#include "bz_internal.h"

struct bz_grammar {
  int num_states = 0;
  std::vector<int32_t> table;      // [num_states * 256], -1 = no transition
  std::vector<uint8_t> accepting;  // [num_states]
  int current = 0;
};

struct bz_device_grammar {
  bz_device* dev = nullptr;
  int num_states = 0;
  long long V = 0;
  uint32_t state = 0;
  int lds_table = 0;                // table staged in LDS by the kernel (num_states <= BZ_GRAMMAR_LDS_MAX_STATES)
  uint16_t* table = nullptr;        // [num_states * 256], 0xFFFF = none
  uint8_t* accepting = nullptr;     // [num_states]
  uint32_t* words = nullptr;        // token bytes, every token padded to a 4-byte boundary, tokens in ascending byte length
  uint32_t* tok_off = nullptr;      // [V] first word of sorted token i
  uint32_t* tok_len = nullptr;      // [V] its byte length
  uint32_t* tok_id = nullptr;       // [V] its index in the caller's vocabulary
  uint32_t* id_off = nullptr;       // [V] the inverse of the sort: first word of caller token t
  uint32_t* id_len = nullptr;       // [V] its byte length
};

// device-resident DFA states, one per row of a decode batch (row r of [N,V] logits); borrows the device grammar
struct bz_grammar_cursor {
  bz_device* dev = nullptr;
  const bz_device_grammar* dg = nullptr;
  int N = 0;
  uint32_t* state = nullptr;        // [N] a state below num_states, or BZ_GRAMMAR_ROW_FREE
  uint32_t* rejected = nullptr;     // [N] bytes without a transition since the row was set
};

namespace {
constexpr uint16_t NONE16 = 0xFFFF;
constexpr int MAX_STATES = 65535;          // ids 0 .. 65534; 0xFFFF is the "no transition" entry of the device table
constexpr size_t MAX_NFA_STATES = 1u << 20;

// ---- text ----------------------------------------------------------------------------------------------------------------------------------
typedef std::vector<uint32_t> Cps;

bool utf8_decode(const char* s, Cps& out) {
  const unsigned char* p = (const unsigned char*)s;
  while (*p) {
    uint32_t c; int n;
    if (*p < 0x80) { c = *p; n = 0; }
    else if ((*p & 0xE0) == 0xC0) { c = *p & 0x1F; n = 1; }
    else if ((*p & 0xF0) == 0xE0) { c = *p & 0x0F; n = 2; }
    else if ((*p & 0xF8) == 0xF0) { c = *p & 0x07; n = 3; }
    else return false;
    p++;
    for (int i = 0; i < n; i++, p++) { if ((*p & 0xC0) != 0x80) return false; c = (c << 6) | (*p & 0x3F); }
    if ((n == 1 && c < 0x80) || (n == 2 && c < 0x800) || (n == 3 && c < 0x10000) || c > 0x10FFFF || (c >= 0xD800 && c <= 0xDFFF)) return false;
    out.push_back(c);
  }
  return true;
}
void utf8_push(std::string& s, uint32_t c) {
  if (c < 0x80) s.push_back((char)c);
  else if (c < 0x800) { s.push_back((char)(0xC0 | (c >> 6))); s.push_back((char)(0x80 | (c & 0x3F))); }
  else if (c < 0x10000) { s.push_back((char)(0xE0 | (c >> 12))); s.push_back((char)(0x80 | ((c >> 6) & 0x3F))); s.push_back((char)(0x80 | (c & 0x3F))); }
  else { s.push_back((char)(0xF0 | (c >> 18))); s.push_back((char)(0x80 | ((c >> 12) & 0x3F))); s.push_back((char)(0x80 | ((c >> 6) & 0x3F))); s.push_back((char)(0x80 | (c & 0x3F))); }
}
std::string utf8_of(const Cps& v, size_t b, size_t e) { std::string s; for (size_t i = b; i < e; i++) utf8_push(s, v[i]); return s; }
// char::is_whitespace (what str::trim strips)
bool is_ws(uint32_t c) {
  return (c >= 9 && c <= 13) || c == 32 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) || c == 0x2028 || c == 0x2029 || c == 0x202F ||
         c == 0x205F || c == 0x3000;
}
void trim(const Cps& v, size_t& b, size_t& e) { while (b < e && is_ws(v[b])) b++; while (e > b && is_ws(v[e - 1])) e--; }
bool is_name_char(uint32_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '-' || c == '_'; }

// one rule line: `name ::= body` with the positions of the trimmed body inside the trimmed line
struct Line { Cps cps; std::string name; size_t body_b, body_e; int lineno; };

// parse_gbnf's outer loop (grammar_parser.rs:47-79): lines(), trim, blank / '#' lines skipped, split at the first "::="
int split_lines(const char* gbnf, std::vector<Line>& out) {
  Cps all;
  if (!utf8_decode(gbnf, all)) BZ_FAIL(BZ_E_INVALID, "grammar_compile: the grammar is not valid UTF-8");
  size_t pos = 0; int lineno = 0;
  while (pos < all.size()) {          // str::lines(): pieces between '\n', a final empty piece is dropped
    size_t e = pos;
    while (e < all.size() && all[e] != '\n') e++;
    lineno++;
    size_t b = pos, t = e;
    pos = e + 1;
    trim(all, b, t);
    if (b == t || all[b] == '#') continue;
    Line ln; ln.cps.assign(all.begin() + b, all.begin() + t); ln.lineno = lineno;
    const Cps& c = ln.cps;
    size_t k = 0; bool found = false;
    for (; k + 3 <= c.size(); k++) if (c[k] == ':' && c[k + 1] == ':' && c[k + 2] == '=') { found = true; break; }
    if (!found) BZ_FAIL(BZ_E_INVALID, "Invalid GBNF rule: %s", utf8_of(c, 0, c.size()).c_str());
    size_t nb = 0, ne = k; trim(c, nb, ne);
    ln.name = utf8_of(c, nb, ne);
    ln.body_b = k + 3; ln.body_e = c.size(); trim(c, ln.body_b, ln.body_e);
    out.push_back(std::move(ln));
  }
  if (out.empty()) BZ_FAIL(BZ_E_INVALID, "No rules found in GBNF grammar");
  return BZ_OK;
}

// ---- NFA / DFA ---------------------------------------------------------------------------------------------------------------------------------
struct Edge { std::bitset<256> on; int to; };
struct Nfa {
  std::vector<std::vector<Edge>> edges;
  std::vector<std::vector<int>> eps;
  std::vector<uint8_t> accepting;
  int add() { edges.emplace_back(); eps.emplace_back(); accepting.push_back(0); return (int)edges.size() - 1; }
  size_t size() const { return edges.size(); }
};

void closure(const Nfa& n, std::vector<int>& set) {
  std::vector<int> stack(set);
  std::vector<uint8_t> seen;   // lazily sized: mode 0 has no epsilon moves
  bool any = false;
  for (int s : set) if (!n.eps[s].empty()) { any = true; break; }
  if (!any) { std::sort(set.begin(), set.end()); set.erase(std::unique(set.begin(), set.end()), set.end()); return; }
  seen.assign(n.size(), 0);
  for (int s : set) seen[s] = 1;
  while (!stack.empty()) {
    const int s = stack.back(); stack.pop_back();
    for (int t : n.eps[s]) if (!seen[t]) { seen[t] = 1; set.push_back(t); stack.push_back(t); }
  }
  std::sort(set.begin(), set.end()); set.erase(std::unique(set.begin(), set.end()), set.end());
}

// subset construction from {start} (grammar.rs:225-270) with the bytes visited in ascending order: states are numbered breadth first
int subset(const Nfa& n, int start, bz_grammar& g, bool eps) {
  std::map<std::vector<int>, int> ids;
  std::vector<std::vector<int>> queue;
  std::vector<int> init{start};
  if (eps) closure(n, init);
  ids[init] = 0; queue.push_back(init);
  g.table.assign(256, -1); g.accepting.assign(1, 0);
  std::vector<int> tg[256];
  for (size_t q = 0; q < queue.size(); q++) {
    const std::vector<int> cur = queue[q];
    for (int s : cur) if (n.accepting[s]) g.accepting[q] = 1;
    for (auto& v : tg) v.clear();
    for (int s : cur) for (const Edge& e : n.edges[s]) for (int b = 0; b < 256; b++) if (e.on[b]) tg[b].push_back(e.to);
    for (int b = 0; b < 256; b++) {
      if (tg[b].empty()) continue;
      std::vector<int>& t = tg[b];
      if (eps) closure(n, t); else { std::sort(t.begin(), t.end()); t.erase(std::unique(t.begin(), t.end()), t.end()); }
      auto it = ids.find(t);
      int id;
      if (it != ids.end()) id = it->second;
      else {
        id = (int)queue.size();
        if (id >= MAX_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: more than %d DFA states", MAX_STATES);
        ids.emplace(t, id); queue.push_back(t);
        g.table.resize((size_t)(id + 1) * 256, -1); g.accepting.push_back(0);
      }
      g.table[q * 256 + b] = id;
    }
  }
  g.num_states = (int)queue.size();
  g.current = 0;
  return BZ_OK;
}

// REGULAR mode: drop transitions into states from which no accepting state is reachable, renumber breadth first / ascending byte
void trim_dead(bz_grammar& g) {
  const int n = g.num_states;
  std::vector<std::vector<int>> rev((size_t)n);
  for (int s = 0; s < n; s++) for (int b = 0; b < 256; b++) { const int t = g.table[(size_t)s * 256 + b]; if (t >= 0) rev[t].push_back(s); }
  std::vector<uint8_t> live((size_t)n, 0);
  std::vector<int> stack;
  for (int s = 0; s < n; s++) if (g.accepting[s]) { live[s] = 1; stack.push_back(s); }
  while (!stack.empty()) { const int s = stack.back(); stack.pop_back(); for (int p : rev[s]) if (!live[p]) { live[p] = 1; stack.push_back(p); } }
  std::vector<int> id((size_t)n, -1), order{0};
  id[0] = 0;
  for (size_t q = 0; q < order.size(); q++)
    for (int b = 0; b < 256; b++) { const int t = g.table[(size_t)order[q] * 256 + b]; if (t >= 0 && live[t] && id[t] < 0) { id[t] = (int)order.size(); order.push_back(t); } }
  bz_grammar o;
  o.num_states = (int)order.size();
  o.table.assign((size_t)o.num_states * 256, -1); o.accepting.assign((size_t)o.num_states, 0);
  for (size_t q = 0; q < order.size(); q++) {
    o.accepting[q] = g.accepting[order[q]];
    for (int b = 0; b < 256; b++) { const int t = g.table[(size_t)order[q] * 256 + b]; if (t >= 0 && live[t]) o.table[q * 256 + b] = id[t]; }
  }
  g = std::move(o);
}

// ---- flags == 0: the reference's parser and compiler ---------------------------------------------------------------------------------------------
struct El0 { int kind; /* 0 literal, 1 class, 2 anything else */ std::string bytes; std::vector<std::pair<uint8_t, uint8_t>> ranges; };

// the escape table of a quoted literal (grammar_parser.rs:95-109); i stands on the character after the backslash
void push_escape(const Cps& c, size_t& i, size_t e, std::string& lit) {
  if (i >= e) return;                       // a backslash at the very end: consumed, nothing pushed
  const uint32_t x = c[i++];
  if (x == 'n') lit.push_back('\n'); else if (x == 't') lit.push_back('\t'); else if (x == '"') lit.push_back('"'); else if (x == '\\') lit.push_back('\\');
  else { lit.push_back('\\'); utf8_push(lit, x); }
}

// parse_gbnf_sequence (grammar_parser.rs:81-190) over c[b, e)
int parse_seq0(const Line& ln, size_t b, size_t e, std::vector<El0>& out) {
  const Cps& c = ln.cps;
  size_t i = b;
  while (i < e) {
    const uint32_t ch0 = c[i];
    if (ch0 == '"') {
      i++;
      El0 el; el.kind = 0;
      while (i < e) {
        const uint32_t ch = c[i];
        if (ch == '"') { i++; break; }
        if (ch == '\\') { i++; push_escape(c, i, e, el.bytes); }
        else { utf8_push(el.bytes, ch); i++; }
      }
      out.push_back(std::move(el));
    } else if (ch0 == '[') {
      i++;
      const bool neg = i < e && c[i] == '^';
      if (neg) i++;
      El0 el; el.kind = neg ? 2 : 1;
      while (i < e) {
        const uint32_t ch = c[i];
        if (ch == ']') { i++; break; }
        const uint8_t start = (uint8_t)ch;      // `ch as u8`
        i++;
        if (i < e && c[i] == '-') {
          i++;
          if (i < e) { el.ranges.emplace_back(start, (uint8_t)c[i]); i++; }   // a ']' here is the END of the range, as in the reference
        } else el.ranges.emplace_back(start, start);
      }
      out.push_back(std::move(el));
    } else if (ch0 == ' ' || ch0 == '\t') {
      i++;
    } else {
      const size_t nb = i;
      while (i < e && is_name_char(c[i])) i++;
      if (i == nb) {
        if (ch0 >= 0x80)
          BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: non-ASCII character outside quotes and brackets (the reference's Unicode name test is not carried)",
                  ln.lineno, nb + 1);
        BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: '%c' is not consumed by the reference's parser (it loops forever there); groups and postfix "
                "operators after a literal or a class need BZ_GRAMMAR_REGULAR", ln.lineno, nb + 1, (char)ch0);
      }
      if (i < e && (c[i] == '*' || c[i] == '+' || c[i] == '?')) i++;
      El0 el; el.kind = 2;
      out.push_back(std::move(el));
    }
  }
  return BZ_OK;
}

int compile0(const std::vector<Line>& lines, bz_grammar& g) {
  // parse every rule (the reference does, so a body it cannot parse fails the whole grammar), expand the first `root`
  std::vector<std::vector<std::vector<El0>>> rules;
  for (const Line& ln : lines) {
    std::vector<std::vector<El0>> alts;
    size_t b = ln.body_b;
    for (;;) {                             // body.split('|'): every '|', quoted or not
      size_t e = b;
      while (e < ln.body_e && ln.cps[e] != '|') e++;
      size_t tb = b, te = e; trim(ln.cps, tb, te);
      alts.emplace_back();
      BZ_TRY(parse_seq0(ln, tb, te, alts.back()));
      if (e >= ln.body_e) break;
      b = e + 1;
    }
    rules.push_back(std::move(alts));
  }
  Nfa n; n.add();
  for (size_t r = 0; r < lines.size(); r++) {
    if (lines[r].name != "root") continue;
    for (const auto& alt : rules[r]) {
      int cur = 0;
      for (const El0& el : alt) {
        if (el.kind == 0) {
          for (unsigned char byte : el.bytes) { const int nx = n.add(); Edge ed; ed.on.set(byte); ed.to = nx; n.edges[cur].push_back(ed); cur = nx; }
        } else {
          const int nx = n.add(); Edge ed; ed.to = nx;
          if (el.kind == 1) { for (auto& rg : el.ranges) for (int byte = rg.first; byte <= rg.second; byte++) ed.on.set(byte); }
          else for (int byte = 0; byte <= 127; byte++) ed.on.set(byte);
          n.edges[cur].push_back(ed); cur = nx;
        }
        if (n.size() > MAX_NFA_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: grammar too large");
      }
      n.accepting[cur] = 1;
    }
    break;
  }
  return subset(n, 0, g, false);
}

// ---- BZ_GRAMMAR_REGULAR ----------------------------------------------------------------------------------------------------------------------------
enum { N_LIT, N_SET, N_SEQ, N_ALT, N_STAR, N_PLUS, N_OPT, N_REF };
struct Node { int kind = N_SEQ; std::string bytes; std::bitset<256> set; std::vector<Node> kids; std::string name; int lineno = 0; size_t col = 0; };

struct RegParser {
  const Line& ln; size_t i, e; int depth = 0;
  RegParser(const Line& l) : ln(l), i(l.body_b), e(l.body_e) {}
  void blanks() { while (i < e && (ln.cps[i] == ' ' || ln.cps[i] == '\t')) i++; }
  int alternation(Node& out, bool in_group) {
    out.kind = N_ALT;
    for (;;) {
      Node seq; seq.kind = N_SEQ;
      BZ_TRY(sequence(seq, in_group));
      out.kids.push_back(std::move(seq));
      if (i < e && ln.cps[i] == '|') { i++; continue; }
      break;
    }
    return BZ_OK;
  }
  int sequence(Node& seq, bool in_group) {
    const Cps& c = ln.cps;
    for (;;) {
      blanks();
      if (i >= e || c[i] == '|') return BZ_OK;
      if (c[i] == ')') {
        if (!in_group) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unbalanced ')'", ln.lineno, i + 1);
        return BZ_OK;
      }
      Node item; item.lineno = ln.lineno; item.col = i + 1;
      const uint32_t ch0 = c[i];
      if (ch0 == '"') {
        i++; item.kind = N_LIT;
        bool closed = false;
        while (i < e) {
          const uint32_t ch = c[i];
          if (ch == '"') { i++; closed = true; break; }
          if (ch == '\\') { i++; push_escape(c, i, e, item.bytes); }
          else { utf8_push(item.bytes, ch); i++; }
        }
        if (!closed) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unterminated literal", ln.lineno, item.col);
      } else if (ch0 == '[') {
        i++; item.kind = N_SET;
        const bool neg = i < e && c[i] == '^';
        if (neg) i++;
        bool closed = false;
        while (i < e) {
          const uint32_t ch = c[i];
          if (ch == ']') { i++; closed = true; break; }
          if (ch >= 0x80) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: non-ASCII class member (classes are sets of bytes)", ln.lineno, i + 1);
          i++;
          uint32_t hi = ch;
          if (i + 1 < e && c[i] == '-' && c[i + 1] != ']') {
            hi = c[i + 1];
            if (hi >= 0x80) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: non-ASCII class member (classes are sets of bytes)", ln.lineno, i + 2);
            i += 2;
          }
          for (uint32_t b = ch; b <= hi; b++) item.set.set(b);
        }
        if (!closed) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unterminated class", ln.lineno, item.col);
        if (neg) item.set.flip();
      } else if (ch0 == '(') {
        i++;
        if (++depth > 200) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d: groups nested too deeply", ln.lineno);
        BZ_TRY(alternation(item, true));
        depth--;
        if (i >= e || c[i] != ')') BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unbalanced '('", ln.lineno, item.col);
        i++;
      } else if (is_name_char(ch0)) {
        const size_t nb = i;
        while (i < e && is_name_char(c[i])) i++;
        item.kind = N_REF; item.name = utf8_of(c, nb, i);
      } else {
        BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unexpected character", ln.lineno, i + 1);
      }
      while (i < e && (c[i] == '*' || c[i] == '+' || c[i] == '?')) {
        Node rep; rep.kind = c[i] == '*' ? N_STAR : (c[i] == '+' ? N_PLUS : N_OPT); rep.lineno = item.lineno; rep.col = item.col;
        rep.kids.push_back(std::move(item));
        item = std::move(rep);
        i++;
      }
      seq.kids.push_back(std::move(item));
    }
  }
};

struct RegBuilder {
  const std::map<std::string, const Node*>& rules;
  Nfa n;
  std::vector<std::string> active;
  RegBuilder(const std::map<std::string, const Node*>& r) : rules(r) {}
  // Thompson fragment of `nd`: entered at *s, left at *t
  int build(const Node& nd, int* s, int* t) {
    if (n.size() > MAX_NFA_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: grammar too large after inlining (more than %zu NFA states)", MAX_NFA_STATES);
    switch (nd.kind) {
      case N_LIT: {
        int cur = n.add(); *s = cur;
        for (unsigned char b : nd.bytes) { const int nx = n.add(); Edge e; e.on.set(b); e.to = nx; n.edges[cur].push_back(e); cur = nx; }
        *t = cur; return BZ_OK;
      }
      case N_SET: {
        *s = n.add(); *t = n.add();
        Edge e; e.on = nd.set; e.to = *t;
        if (nd.set.any()) n.edges[*s].push_back(e);
        return BZ_OK;
      }
      case N_SEQ: {
        int cur = n.add(); *s = cur;
        for (const Node& k : nd.kids) { int a, b; BZ_TRY(build(k, &a, &b)); n.eps[cur].push_back(a); cur = b; }
        *t = cur; return BZ_OK;
      }
      case N_ALT: {
        *s = n.add(); const int end = n.add();
        for (const Node& k : nd.kids) { int a, b; BZ_TRY(build(k, &a, &b)); n.eps[*s].push_back(a); n.eps[b].push_back(end); }
        *t = end; return BZ_OK;
      }
      case N_STAR: case N_PLUS: case N_OPT: {
        *s = n.add(); const int end = n.add();
        int a, b; BZ_TRY(build(nd.kids[0], &a, &b));
        n.eps[*s].push_back(a); n.eps[b].push_back(end);
        if (nd.kind != N_PLUS) n.eps[*s].push_back(end);
        if (nd.kind != N_OPT) n.eps[b].push_back(a);
        *t = end; return BZ_OK;
      }
      case N_REF: {
        auto it = rules.find(nd.name);
        if (it == rules.end()) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: rule '%s' is not defined", nd.lineno, nd.col, nd.name.c_str());
        for (const std::string& a : active)
          if (a == nd.name) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: rule '%s' is recursive (only the regular subset of GBNF is compiled)", nd.name.c_str());
        active.push_back(nd.name);
        const int rc = build(*it->second, s, t);
        active.pop_back();
        return rc;
      }
    }
    BZ_FAIL(BZ_E_INVALID, "grammar_compile: internal error");
  }
};

int compile_regular(const std::vector<Line>& lines, bz_grammar& g) {
  std::vector<Node> bodies(lines.size());
  std::map<std::string, const Node*> rules;
  for (size_t r = 0; r < lines.size(); r++) {
    RegParser p(lines[r]);
    BZ_TRY(p.alternation(bodies[r], false));
    if (p.i < p.e) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: line %d column %zu: unbalanced ')'", lines[r].lineno, p.i + 1);
  }
  for (size_t r = 0; r < lines.size(); r++) rules.emplace(lines[r].name, &bodies[r]);   // the first definition of a name wins, as for `root` in mode 0
  if (!rules.count("root")) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_compile: rule 'root' is not defined");
  RegBuilder b(rules);
  b.active.push_back("root");
  int s, t;
  BZ_TRY(b.build(*rules["root"], &s, &t));
  b.n.accepting[t] = 1;
  BZ_TRY(subset(b.n, s, g, true));
  trim_dead(g);
  return BZ_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// host API
// ---------------------------------------------------------------------------------------------------------------------------------------------------
extern "C" int bz_grammar_compile(const char* gbnf, uint32_t flags, bz_grammar** out) {
  BZ_API_BEGIN
  if (!gbnf || !out) BZ_FAIL(BZ_E_INVALID, "grammar_compile: null argument");
  if (flags & ~(uint32_t)BZ_GRAMMAR_REGULAR) BZ_FAIL(BZ_E_INVALID, "grammar_compile: unknown flag bits 0x%x", flags);
  std::vector<Line> lines;
  BZ_TRY(split_lines(gbnf, lines));
  std::unique_ptr<bz_grammar> g(new bz_grammar());
  if (flags & BZ_GRAMMAR_REGULAR) BZ_TRY(compile_regular(lines, *g)); else BZ_TRY(compile0(lines, *g));
  *out = g.release();
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_from_table(int num_states, const int32_t* table, const uint8_t* accepting, bz_grammar** out) {
  BZ_API_BEGIN
  if (!table || !accepting || !out || num_states <= 0) BZ_FAIL(BZ_E_INVALID, "grammar_from_table: bad argument");
  if (num_states > MAX_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_from_table: more than %d states", MAX_STATES);
  for (size_t i = 0; i < (size_t)num_states * 256; i++)
    if (table[i] < -1 || table[i] >= num_states) BZ_FAIL(BZ_E_INVALID, "grammar_from_table: entry %d at state %zu byte %zu is not -1 or a state below %d", table[i], i / 256, i % 256, num_states);
  std::unique_ptr<bz_grammar> g(new bz_grammar());
  g->num_states = num_states;
  g->table.assign(table, table + (size_t)num_states * 256);
  g->accepting.resize((size_t)num_states);
  for (int s = 0; s < num_states; s++) g->accepting[s] = accepting[s] ? 1 : 0;
  *out = g.release();
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_table(const bz_grammar* g, int32_t* table_out, uint8_t* accepting_out) {
  BZ_API_BEGIN
  if (!g) BZ_FAIL(BZ_E_INVALID, "grammar_table: null grammar");
  if (table_out) memcpy(table_out, g->table.data(), g->table.size() * 4);
  if (accepting_out) memcpy(accepting_out, g->accepting.data(), g->accepting.size());
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_num_states(const bz_grammar* g) { return g ? g->num_states : BZ_E_INVALID; }
extern "C" int bz_grammar_current_state(const bz_grammar* g) { return g ? g->current : BZ_E_INVALID; }
extern "C" int bz_grammar_is_accepting(const bz_grammar* g) { return g ? (int)g->accepting[g->current] : BZ_E_INVALID; }
extern "C" int bz_grammar_reset(bz_grammar* g) { if (!g) return BZ_E_INVALID; g->current = 0; return BZ_OK; }
extern "C" int bz_grammar_free(bz_grammar* g) { delete g; return BZ_OK; }

// GrammarDfa::advance per byte as the generate loop calls it (executor_generate.rs:159-161): the result of advance() is ignored there, so a byte
// without a transition leaves the state where it is and the next byte is tried from it
extern "C" int bz_grammar_advance(bz_grammar* g, const uint8_t* bytes, size_t n, int* n_rejected) {
  BZ_API_BEGIN
  if (!g || (!bytes && n)) BZ_FAIL(BZ_E_INVALID, "grammar_advance: bad argument");
  int rej = 0;
  for (size_t i = 0; i < n; i++) {
    const int32_t nx = g->table[(size_t)g->current * 256 + bytes[i]];
    if (nx >= 0) g->current = nx; else rej++;
  }
  if (n_rejected) *n_rejected = rej;
  return BZ_OK;
  BZ_API_END
}

// n DFAs as one: the tables stacked, every transition shifted by its grammar's offset.  No state of block i reaches another block, so a row's
// state alone decides which language it is in.
extern "C" int bz_grammar_concat(const bz_grammar* const* gs, int n, bz_grammar** out, int32_t* starts) {
  BZ_API_BEGIN
  if (!gs || !out || !starts || n < 1) BZ_FAIL(BZ_E_INVALID, "grammar_concat: bad argument (n >= 1 grammars, out and starts[n] required)");
  long long total = 0;
  for (int i = 0; i < n; i++) {
    if (!gs[i]) BZ_FAIL(BZ_E_INVALID, "grammar_concat: grammar %d is null", i);
    total += gs[i]->num_states;
  }
  if (total > MAX_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_concat: %lld states in total, more than %d", total, MAX_STATES);
  std::unique_ptr<bz_grammar> g(new bz_grammar());
  g->num_states = (int)total;
  g->table.reserve((size_t)total * 256); g->accepting.reserve((size_t)total);
  int32_t off = 0;
  for (int i = 0; i < n; i++) {
    starts[i] = off;
    for (int32_t t : gs[i]->table) g->table.push_back(t < 0 ? -1 : t + off);
    g->accepting.insert(g->accepting.end(), gs[i]->accepting.begin(), gs[i]->accepting.end());
    off += gs[i]->num_states;
  }
  g->current = starts[0];
  *out = g.release();
  return BZ_OK;
  BZ_API_END
}

static int check_vocab(const char* who, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V) {
  if (!offsets || V <= 0) BZ_FAIL(BZ_E_INVALID, "%s: offsets[V+1] with V > 0 required", who);
  if (offsets[0] != 0) BZ_FAIL(BZ_E_INVALID, "%s: offsets[0] must be 0", who);
  for (int64_t i = 0; i < V; i++) if (offsets[i + 1] < offsets[i]) BZ_FAIL(BZ_E_INVALID, "%s: offsets must not decrease (token %lld)", who, (long long)i);
  if (offsets[V] > 0 && !vocab_bytes) BZ_FAIL(BZ_E_INVALID, "%s: null vocab_bytes", who);
  if (offsets[V] > 0x7fffffffLL) BZ_FAIL(BZ_E_UNSUPPORTED, "%s: more than 2 GiB of token bytes", who);
  return BZ_OK;
}

// bz_grammar_advance over the bytes of each token in turn (the generate loop's rule: a byte without a transition leaves the state in place and is counted)
extern "C" int bz_grammar_advance_tokens(bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, const int64_t* tokens, int64_t n, int* n_rejected) {
  BZ_API_BEGIN
  if (!g || n < 0 || (!tokens && n)) BZ_FAIL(BZ_E_INVALID, "grammar_advance_tokens: bad argument");
  BZ_TRY(check_vocab("grammar_advance_tokens", vocab_bytes, offsets, V));
  for (int64_t i = 0; i < n; i++)
    if (tokens[i] < 0 || tokens[i] >= V) BZ_FAIL(BZ_E_INVALID, "grammar_advance_tokens: token %lld at index %lld is outside the vocabulary [0,%lld)", (long long)tokens[i], (long long)i, (long long)V);
  int rej = 0;
  for (int64_t i = 0; i < n; i++)
    for (int64_t k = offsets[tokens[i]]; k < offsets[tokens[i] + 1]; k++) {
      const int32_t nx = g->table[(size_t)g->current * 256 + vocab_bytes[k]];
      if (nx >= 0) g->current = nx; else rej++;
    }
  if (n_rejected) *n_rejected = rej;
  return BZ_OK;
  BZ_API_END
}

// compute_token_mask (grammar.rs:69-84); a token without bytes is allowed in every state
extern "C" int bz_grammar_token_mask(const bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, uint8_t* allowed_out) {
  BZ_API_BEGIN
  if (!g || !allowed_out) BZ_FAIL(BZ_E_INVALID, "grammar_token_mask: null argument");
  BZ_TRY(check_vocab("grammar_token_mask", vocab_bytes, offsets, V));
  for (int64_t i = 0; i < V; i++) {
    int32_t s = g->current;
    for (int64_t k = offsets[i]; k < offsets[i + 1] && s >= 0; k++) s = g->table[(size_t)s * 256 + vocab_bytes[k]];
    allowed_out[i] = s >= 0;
  }
  return BZ_OK;
  BZ_API_END
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// device: DeviceGrammarDfa + the mask kernel
// ---------------------------------------------------------------------------------------------------------------------------------------------------
// One lane per token, tokens in ascending byte length so that the 64 lanes of a wave walk strings of similar length and leave the loop together.
// A lane walks its token from `state`, one dependent table look-up per byte, and stops at the first missing transition: in a constrained state nearly
// every lane stops at its first byte.  Bytes arrive as aligned 32-bit words (every token starts on a word boundary).  LDS == true: the whole table
// (512 B per state) is staged into LDS first with 16-byte loads -- at most 64 KiB, so two workgroups fit in a CU's 160 KiB; LDS == false: the look-ups
// go through L1 / L2.  Only disallowed tokens are written (a plain vector store of -inf); every other logit keeps its bits because it is never touched.
template <bool LDS>
__global__ __launch_bounds__(256) void k_grammar_mask(float* __restrict__ row, const uint16_t* __restrict__ table, int num_states, unsigned state, const uint32_t* __restrict__ words,
                                                      const uint32_t* __restrict__ tok_off, const uint32_t* __restrict__ tok_len, const uint32_t* __restrict__ tok_id, long long V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  const uint16_t* T = table;
  if (LDS) {
    uint4* dst = (uint4*)g_smem;
    const uint4* src = (const uint4*)table;            // hipMalloc'd: 256-byte aligned; 512 B per state = 32 uint4
    const int n16 = num_states * 32;
    for (int k = threadIdx.x; k < n16; k += 256) dst[k] = src[k];
    __syncthreads();
    T = (const uint16_t*)g_smem;
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  const unsigned len = tok_len[i];
  if (len == 0) return;                                // a token without bytes is allowed in every state
  const uint32_t* w = words + tok_off[i];
  unsigned s = state;
  bool dead = false;
  for (unsigned k = 0; k < len && !dead; k += 4) {
    unsigned word = w[k >> 2];
    const unsigned nb = min(4u, len - k);
    for (unsigned j = 0; j < nb; j++) {
      s = T[s * 256u + (word & 0xffu)];
      if (s == NONE16) { dead = true; break; }
      word >>= 8;
    }
  }
  if (dead) row[tok_id[i]] = __uint_as_float(0xff800000u);
}

// The same walk for the N rows of a decode batch, every row from its own device-resident state.  A workgroup owns 256 tokens (grid.x) and a chunk of
// `rows_per_wg` rows (grid.y): it stages the table once and serves every row of its chunk with it, so the staging is paid once per chunk, not once per
// row.  A lane reads its token's length, id and first word once; in a constrained state nearly every lane dies inside that word.  state[r] is one uniform
// load; a FREE row (or any value that is no state) is skipped without touching its logits.
template <bool LDS>
__global__ __launch_bounds__(256) void k_grammar_mask_rows(float* __restrict__ logits, const uint16_t* __restrict__ table, int num_states, const uint32_t* __restrict__ state, int N,
                                                           int rows_per_wg, const uint32_t* __restrict__ words, const uint32_t* __restrict__ tok_off,
                                                           const uint32_t* __restrict__ tok_len, const uint32_t* __restrict__ tok_id, long long V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  const uint16_t* T = table;
  if (LDS) {
    uint4* dst = (uint4*)g_smem;
    const uint4* src = (const uint4*)table;
    const int n16 = num_states * 32;
    for (int k = threadIdx.x; k < n16; k += 256) dst[k] = src[k];
    __syncthreads();
    T = (const uint16_t*)g_smem;
  }
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  const unsigned len = tok_len[i];
  if (len == 0) return;                                // a token without bytes is allowed in every state
  const uint32_t* w = words + tok_off[i];
  const unsigned w0 = w[0];
  const size_t id = tok_id[i];
  const int r0 = blockIdx.y * rows_per_wg, r1 = min(N, r0 + rows_per_wg);
  for (int r = r0; r < r1; r++) {
    unsigned s = state[r];
    if (s >= (unsigned)num_states) continue;           // BZ_GRAMMAR_ROW_FREE
    bool dead = false;
    for (unsigned k = 0; k < len && !dead; k += 4) {
      unsigned word = k ? w[k >> 2] : w0;
      const unsigned nb = min(4u, len - k);
      for (unsigned j = 0; j < nb; j++) {
        s = T[s * 256u + (word & 0xffu)];
        if (s == NONE16) { dead = true; break; }
        word >>= 8;
      }
    }
    if (dead) logits[(size_t)r * (size_t)V + id] = __uint_as_float(0xff800000u);
  }
}

// One lane per row: the sampled token's bytes (found through the inverse of the length sort) walked through the global table with the generate loop's
// rule.  A FREE row, an id outside [0, V) and a token without bytes change nothing.  Lane r reads and writes row r only.
__global__ __launch_bounds__(64) void k_grammar_advance_rows(uint32_t* __restrict__ state, uint32_t* __restrict__ rejected, const long long* __restrict__ tokens, int N,
                                                             const uint16_t* __restrict__ table, int num_states, const uint32_t* __restrict__ words,
                                                             const uint32_t* __restrict__ id_off, const uint32_t* __restrict__ id_len, long long V) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= N) return;
  unsigned s = state[r];
  if (s >= (unsigned)num_states) return;
  const long long t = tokens[r];
  if (t < 0 || t >= V) return;
  const unsigned len = id_len[t];
  if (len == 0) return;
  const uint32_t* w = words + id_off[t];
  unsigned rej = 0;
  for (unsigned k = 0; k < len; k += 4) {
    unsigned word = w[k >> 2];
    const unsigned nb = min(4u, len - k);
    for (unsigned j = 0; j < nb; j++) {
      const unsigned nx = table[s * 256u + (word & 0xffu)];
      if (nx == NONE16) rej++; else s = nx;
      word >>= 8;
    }
  }
  state[r] = s;
  if (rej) rejected[r] += rej;
}

extern "C" int bz_grammar_to_device(bz_device* dev, const bz_grammar* g, const uint8_t* vocab_bytes, const int64_t* offsets, int64_t V, bz_device_grammar** out) {
  BZ_API_BEGIN
  if (!dev || !g || !out) BZ_FAIL(BZ_E_INVALID, "grammar_to_device: null argument");
  BZ_TRY(check_vocab("grammar_to_device", vocab_bytes, offsets, V));
  if (V > 0x7fffffffLL) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_to_device: vocab too large");
  if (g->num_states > MAX_STATES) BZ_FAIL(BZ_E_UNSUPPORTED, "grammar_to_device: more than %d states", MAX_STATES);
  // host images: u16 table, tokens sorted by byte length (stable: equal lengths keep the caller's order), bytes padded to words
  std::vector<uint16_t> t16((size_t)g->num_states * 256);
  for (size_t i = 0; i < t16.size(); i++) t16[i] = g->table[i] < 0 ? NONE16 : (uint16_t)g->table[i];
  std::vector<uint32_t> id((size_t)V), off((size_t)V), len((size_t)V);
  for (int64_t i = 0; i < V; i++) id[i] = (uint32_t)i;
  std::stable_sort(id.begin(), id.end(), [&](uint32_t a, uint32_t b) { return offsets[a + 1] - offsets[a] < offsets[b + 1] - offsets[b]; });
  std::vector<uint32_t> words;
  words.reserve((size_t)(offsets[V] / 4 + V));
  for (int64_t i = 0; i < V; i++) {
    const int64_t b = offsets[id[i]], n = offsets[id[i] + 1] - b;
    off[i] = (uint32_t)words.size(); len[i] = (uint32_t)n;
    for (int64_t k = 0; k < n; k += 4) {
      uint32_t wv = 0;
      for (int64_t j = 0; j < 4 && k + j < n; j++) wv |= (uint32_t)vocab_bytes[b + k + j] << (8 * j);
      words.push_back(wv);
    }
  }
  if (words.empty()) words.push_back(0);     // as the reference: at least one element
  std::vector<uint32_t> ioff((size_t)V), ilen((size_t)V);   // the inverse of the sort: what a sampled token id needs to find its bytes
  for (int64_t i = 0; i < V; i++) { ioff[id[i]] = off[i]; ilen[id[i]] = len[i]; }
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  std::unique_ptr<bz_device_grammar> dg(new bz_device_grammar());
  dg->num_states = g->num_states; dg->V = V; dg->state = (uint32_t)g->current;
  dg->lds_table = g->num_states <= BZ_GRAMMAR_LDS_MAX_STATES;
  int rc = BZ_OK;
  auto up = [&](void** p, const void* h, size_t bytes) {
    if (rc != BZ_OK) return;
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) e = hipMemcpy(*p, h, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { bz_set_error("grammar_to_device: %s", hipGetErrorString(e)); rc = e == hipErrorOutOfMemory ? BZ_E_OOM : BZ_E_HIP; }
  };
  up((void**)&dg->table, t16.data(), t16.size() * 2);
  up((void**)&dg->accepting, g->accepting.data(), g->accepting.size());
  up((void**)&dg->words, words.data(), words.size() * 4);
  up((void**)&dg->tok_off, off.data(), off.size() * 4);
  up((void**)&dg->tok_len, len.data(), len.size() * 4);
  up((void**)&dg->tok_id, id.data(), id.size() * 4);
  up((void**)&dg->id_off, ioff.data(), ioff.size() * 4);
  up((void**)&dg->id_len, ilen.data(), ilen.size() * 4);
  if (rc != BZ_OK) {
    hipFree(dg->table); hipFree(dg->accepting); hipFree(dg->words); hipFree(dg->tok_off); hipFree(dg->tok_len); hipFree(dg->tok_id); hipFree(dg->id_off); hipFree(dg->id_len);
    return rc;
  }
  dg->dev = dev;
  bz_dev_retain(dev);
  *out = dg.release();
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_device_grammar_set_state(bz_device_grammar* dg, uint32_t state) {
  BZ_API_BEGIN
  if (!dg) BZ_FAIL(BZ_E_INVALID, "device_grammar_set_state: null grammar");
  if (state >= (uint32_t)dg->num_states) BZ_FAIL(BZ_E_INVALID, "device_grammar_set_state: state %u out of range [0,%d)", state, dg->num_states);
  dg->state = state;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_device_grammar_info(const bz_device_grammar* dg, int32_t* num_states, int64_t* vocab, uint32_t* state, int32_t* lds_table) {
  BZ_API_BEGIN
  if (!dg) BZ_FAIL(BZ_E_INVALID, "device_grammar_info: null grammar");
  if (num_states) *num_states = dg->num_states;
  if (vocab) *vocab = dg->V;
  if (state) *state = dg->state;
  if (lds_table) *lds_table = dg->lds_table;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_device_grammar_free(bz_device_grammar* dg) {
  BZ_API_BEGIN
  if (!dg) return BZ_OK;
  hipStreamSynchronize(dg->dev->stream);
  hipFree(dg->table); hipFree(dg->accepting); hipFree(dg->words); hipFree(dg->tok_off); hipFree(dg->tok_len); hipFree(dg->tok_id); hipFree(dg->id_off); hipFree(dg->id_len);
  bz_dev_release(dg->dev);
  delete dg;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_dfa_mask_logits(bz_device* dev, const bz_tensor* logits, int64_t rows, int64_t vocab, const bz_device_grammar* dg, bz_tensor* logits_out) {
  BZ_API_BEGIN
  if (!dev || !logits || !dg || !logits_out || rows <= 0 || vocab <= 0) BZ_FAIL(BZ_E_INVALID, "grammar_dfa_mask_logits: bad argument");
  if (vocab != dg->V) BZ_FAIL(BZ_E_INVALID, "grammar_dfa_mask_logits: vocab %lld but the grammar was uploaded for %lld tokens", (long long)vocab, dg->V);
  if (dg->dev != dev) BZ_FAIL(BZ_E_INVALID, "grammar_dfa_mask_logits: the grammar lives on another device handle");
  const size_t bytes = (size_t)rows * (size_t)vocab * 4;
  if (logits->dtype != BZ_F32 || logits->nbytes < bytes || logits_out->dtype != BZ_F32 || logits_out->nbytes < bytes)
    BZ_FAIL(BZ_E_INVALID, "grammar_dfa_mask_logits: logits and logits_out must be F32 [rows,vocab]");
  if (dg->state >= (uint32_t)dg->num_states) BZ_FAIL(BZ_E_INVALID, "grammar_dfa_mask_logits: state out of range");
  std::lock_guard<std::mutex> dlock__(dev->mu);
  BZ_HIP(hipSetDevice(dev->id));
  hipStream_t s = dev->stream;
  if (logits_out->ptr != logits->ptr) BZ_HIP(hipMemcpyAsync(logits_out->ptr, logits->ptr, bytes, hipMemcpyDeviceToDevice, s));   // every row, bit for bit; the last one is masked in place below
  float* row = (float*)logits_out->ptr + (size_t)(rows - 1) * (size_t)vocab;
  const unsigned grid = (unsigned)((vocab + 255) / 256);
  const double algo = (double)vocab * 16.0;
  if (dg->lds_table) {
    static bool attr_done = false;
    if (!attr_done) { BZ_HIP(hipFuncSetAttribute((const void*)k_grammar_mask<true>, hipFuncAttributeMaxDynamicSharedMemorySize, BZ_GRAMMAR_LDS_MAX_STATES * 512)); attr_done = true; }
    BZ_LAUNCH("grammar_mask<lds>", algo, (k_grammar_mask<true>), dim3(grid), dim3(256), (size_t)dg->num_states * 512, s, row, (const uint16_t*)dg->table, dg->num_states, dg->state,
              (const uint32_t*)dg->words, (const uint32_t*)dg->tok_off, (const uint32_t*)dg->tok_len, (const uint32_t*)dg->tok_id, (long long)vocab);
  } else {
    BZ_LAUNCH("grammar_mask<global>", algo, (k_grammar_mask<false>), dim3(grid), dim3(256), 0, s, row, (const uint16_t*)dg->table, dg->num_states, dg->state,
              (const uint32_t*)dg->words, (const uint32_t*)dg->tok_off, (const uint32_t*)dg->tok_len, (const uint32_t*)dg->tok_id, (long long)vocab);
  }
  BZ_HIP(hipGetLastError());
  return BZ_OK;
  BZ_API_END
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// the cursor: one device-resident DFA state per row
// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Rows one workgroup of k_grammar_mask_rows serves with one staged table.  64 keeps a batch of up to 64 rows in a one-dimensional grid (the table is
// staged 501 times at V = 128256, as for one row) and gives N = 512 eight chunks.  Reasoned, not tuned: DESIGN.md 6 has the figures, which favour smaller chunks at N = 64.
static const int ROWS_PER_WG = 64;

int bzk_grammar_cursor_dims(const bz_grammar_cursor* c, int* N, long long* V, bz_device** dev) { *N = c->N; *V = c->dg->V; *dev = c->dev; return BZ_OK; }

int bzk_grammar_mask_rows(hipStream_t st, bz_grammar_cursor* c, float* logits) {
  const bz_device_grammar* dg = c->dg;
  const dim3 grid((unsigned)((dg->V + 255) / 256), (unsigned)((c->N + ROWS_PER_WG - 1) / ROWS_PER_WG));
  if (dg->lds_table)
    hipLaunchKernelGGL((k_grammar_mask_rows<true>), grid, dim3(256), (size_t)dg->num_states * 512, st, logits, (const uint16_t*)dg->table, dg->num_states, (const uint32_t*)c->state, c->N,
                       ROWS_PER_WG, (const uint32_t*)dg->words, (const uint32_t*)dg->tok_off, (const uint32_t*)dg->tok_len, (const uint32_t*)dg->tok_id, dg->V);
  else
    hipLaunchKernelGGL((k_grammar_mask_rows<false>), grid, dim3(256), 0, st, logits, (const uint16_t*)dg->table, dg->num_states, (const uint32_t*)c->state, c->N, ROWS_PER_WG,
                       (const uint32_t*)dg->words, (const uint32_t*)dg->tok_off, (const uint32_t*)dg->tok_len, (const uint32_t*)dg->tok_id, dg->V);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

int bzk_grammar_advance_rows(hipStream_t st, bz_grammar_cursor* c, const long long* tokens) {
  const bz_device_grammar* dg = c->dg;
  hipLaunchKernelGGL(k_grammar_advance_rows, dim3((c->N + 63) / 64), dim3(64), 0, st, c->state, c->rejected, tokens, c->N, (const uint16_t*)dg->table, dg->num_states,
                     (const uint32_t*)dg->words, (const uint32_t*)dg->id_off, (const uint32_t*)dg->id_len, dg->V);
  BZ_HIP(hipGetLastError());
  return BZ_OK;
}

extern "C" int bz_grammar_cursor_free(bz_grammar_cursor* c) {
  BZ_API_BEGIN
  if (!c) return BZ_OK;
  if (c->dev) { hipSetDevice(c->dev->id); hipStreamSynchronize(c->dev->stream); }
  if (c->state) hipFree(c->state);
  if (c->rejected) hipFree(c->rejected);
  if (c->dev) bz_dev_release(c->dev);
  delete c;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_cursor_create(const bz_device_grammar* dg, int N, bz_grammar_cursor** out) {
  BZ_API_BEGIN
  if (!out) BZ_FAIL(BZ_E_INVALID, "grammar cursor create: null output pointer");
  *out = nullptr;
  if (!dg) BZ_FAIL(BZ_E_INVALID, "grammar cursor create: null device grammar");
  if (N < 1 || N > 512) BZ_FAIL(BZ_E_INVALID, "grammar cursor create: N = %d out of range (1 <= N <= 512)", N);
  if (dg->state >= (uint32_t)dg->num_states) BZ_FAIL(BZ_E_INVALID, "grammar cursor create: the grammar's state is out of range");
  std::lock_guard<std::mutex> dlock__(dg->dev->mu);
  BZ_HIP(hipSetDevice(dg->dev->id));
  // dynamic LDS beyond the default needs the attribute; set here so that no capture ever contains the call
  if (dg->lds_table) BZ_HIP(hipFuncSetAttribute((const void*)k_grammar_mask_rows<true>, hipFuncAttributeMaxDynamicSharedMemorySize, BZ_GRAMMAR_LDS_MAX_STATES * 512));
  bz_grammar_cursor* c = new bz_grammar_cursor();
  bz_dev_retain(dg->dev); c->dev = dg->dev;
  c->dg = dg; c->N = N;
  std::vector<uint32_t> init((size_t)N, dg->state);
  if (hipMalloc(&c->state, (size_t)N * 4) != hipSuccess || hipMalloc(&c->rejected, (size_t)N * 4) != hipSuccess) {
    (void)hipGetLastError(); bz_grammar_cursor_free(c); BZ_FAIL(BZ_E_OOM, "grammar cursor create: out of device memory");
  }
  if (hipMemcpy(c->state, init.data(), (size_t)N * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(c->rejected, 0, (size_t)N * 4) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    bz_grammar_cursor_free(c); BZ_FAIL(BZ_E_HIP, "grammar cursor create: upload failed");
  }
  *out = c;
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_cursor_set_row(bz_grammar_cursor* c, int row, uint32_t state) {
  BZ_API_BEGIN
  if (!c) BZ_FAIL(BZ_E_INVALID, "grammar cursor set_row: null cursor");
  if (row < 0 || row >= c->N) BZ_FAIL(BZ_E_INVALID, "grammar cursor set_row: row %d out of range (N = %d)", row, c->N);
  if (state != BZ_GRAMMAR_ROW_FREE && state >= (uint32_t)c->dg->num_states)
    BZ_FAIL(BZ_E_INVALID, "grammar cursor set_row: state %u is neither below the grammar's %d states nor BZ_GRAMMAR_ROW_FREE", state, c->dg->num_states);
  const uint32_t zero = 0;
  std::lock_guard<std::mutex> dlock__(c->dev->mu);
  BZ_HIP(hipSetDevice(c->dev->id));
  BZ_HIP(hipMemcpyAsync(c->state + row, &state, 4, hipMemcpyHostToDevice, c->dev->stream));   // stream-ordered: after the replays already enqueued
  BZ_HIP(hipMemcpyAsync(c->rejected + row, &zero, 4, hipMemcpyHostToDevice, c->dev->stream));
  BZ_HIP(hipStreamSynchronize(c->dev->stream));
  return BZ_OK;
  BZ_API_END
}

// what the request engine needs: the states (k_engine_finish frees a row that ends) and set_row without the wait (`stage`: pinned, two words)
uint32_t* bzk_grammar_cursor_states(bz_grammar_cursor* c) { return c->state; }
int bzk_grammar_cursor_num_states(const bz_grammar_cursor* c) { return c->dg->num_states; }
int bzk_grammar_cursor_stage_row(hipStream_t st, bz_grammar_cursor* c, int row, uint32_t state, uint32_t* stage) {
  stage[0] = state; stage[1] = 0;
  BZ_HIP(hipMemcpyAsync(c->state + row, stage, 4, hipMemcpyHostToDevice, st));
  BZ_HIP(hipMemcpyAsync(c->rejected + row, stage + 1, 4, hipMemcpyHostToDevice, st));
  return BZ_OK;
}

extern "C" int bz_grammar_cursor_read(bz_grammar_cursor* c, uint32_t* states, uint32_t* rejected) {
  BZ_API_BEGIN
  if (!c || !states) BZ_FAIL(BZ_E_INVALID, "grammar cursor read: null argument");
  std::lock_guard<std::mutex> dlock__(c->dev->mu);
  BZ_HIP(hipSetDevice(c->dev->id));
  BZ_HIP(hipMemcpyAsync(states, c->state, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->dev->stream));
  if (rejected) BZ_HIP(hipMemcpyAsync(rejected, c->rejected, (size_t)c->N * 4, hipMemcpyDeviceToHost, c->dev->stream));
  BZ_HIP(hipStreamSynchronize(c->dev->stream));
  return BZ_OK;
  BZ_API_END
}

extern "C" int bz_grammar_cursor_mask(bz_grammar_cursor* c, bz_tensor* logits) {
  BZ_API_BEGIN
  if (!c || !logits) BZ_FAIL(BZ_E_INVALID, "grammar cursor mask: null argument");
  const size_t N = (size_t)c->N, V = (size_t)c->dg->V;
  if (logits->dtype != BZ_F32 || logits->nbytes != N * V * 4) BZ_FAIL(BZ_E_INVALID, "grammar cursor mask: logits must be F32 [%zu,%zu] (got dtype %d, %zu bytes)", N, V, logits->dtype, logits->nbytes);
  if (logits->dev != c->dev) BZ_FAIL(BZ_E_INVALID, "grammar cursor mask: the logits live on another device handle");
  std::lock_guard<std::mutex> dlock__(c->dev->mu);
  BZ_HIP(hipSetDevice(c->dev->id));
  return bzk_grammar_mask_rows(c->dev->stream, c, (float*)logits->ptr);
  BZ_API_END
}

extern "C" int bz_grammar_cursor_advance(bz_grammar_cursor* c, const bz_tensor* tokens) {
  BZ_API_BEGIN
  if (!c || !tokens) BZ_FAIL(BZ_E_INVALID, "grammar cursor advance: null argument");
  if (tokens->dtype != BZ_I64 || tokens->nbytes != (size_t)c->N * 8) BZ_FAIL(BZ_E_INVALID, "grammar cursor advance: tokens must be I64 [%d] (got dtype %d, %zu bytes)", c->N, tokens->dtype, tokens->nbytes);
  if (tokens->dev != c->dev) BZ_FAIL(BZ_E_INVALID, "grammar cursor advance: the tokens live on another device handle");
  std::lock_guard<std::mutex> dlock__(c->dev->mu);
  BZ_HIP(hipSetDevice(c->dev->id));
  return bzk_grammar_advance_rows(c->dev->stream, c, (const long long*)tokens->ptr);
  BZ_API_END
}
