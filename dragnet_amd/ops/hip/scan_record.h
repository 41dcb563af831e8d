// Record layer of the scan engine: a record's bytes and a PlanView in,
// captured field values (FV) and predicate results out.  Plain C++17 as
// well, like scan_text.h: the host checker plays lane 0 of one block.
#pragma once
#include "scan_text.h"

namespace dn {

constexpr int BLOCK = 256;
constexpr int SIG_DEPTH = 6;      // max dotted-path components

// -------------------------------------------------------------------
// per-record extracted field values, stored in LDS (SoA, [field][tid])

struct FV {
  // (soff, slen) double as the VALUE bits for T_NUM slots — a slot is
  // either a span (str/obj/arr) or a number, never both, and every
  // get_num consumer is type-gated.  The union halves the per-field
  // LDS footprint (9 B/field/thread), which buys occupancy: LDS is
  // the block-count limiter on this kernel.
  uint8_t* type;   // nf * BLOCK
  uint32_t* soff;  // nf * BLOCK; T_NUM: low 32 bits of the double
  uint32_t* slen;  // nf * BLOCK; T_NUM: high 32 bits
  int tid;
  DN_HD_INLINE void set(int f, uint8_t t, uint32_t off, uint32_t len,
                        double n) {
    type[f * BLOCK + tid] = t;
    if (t == T_NUM) {
      uint64_t b = (uint64_t)DN_DOUBLE_AS_LL(n);
      soff[f * BLOCK + tid] = (uint32_t)b;
      slen[f * BLOCK + tid] = (uint32_t)(b >> 32);
    } else {
      soff[f * BLOCK + tid] = off;
      slen[f * BLOCK + tid] = len;
    }
  }
  DN_HD_INLINE void set_len(int f, uint32_t len) {
    slen[f * BLOCK + tid] = len;
  }
  DN_HD_INLINE uint8_t get_type(int f) const { return type[f * BLOCK + tid]; }
  DN_HD_INLINE uint32_t get_soff(int f) const { return soff[f * BLOCK + tid]; }
  DN_HD_INLINE uint32_t get_slen(int f) const { return slen[f * BLOCK + tid]; }
  DN_HD_INLINE double get_num(int f) const {
    uint64_t b = (uint64_t)soff[f * BLOCK + tid]
               | ((uint64_t)slen[f * BLOCK + tid] << 32);
    return DN_LL_AS_DOUBLE((long long)b);
  }
};

// -------------------------------------------------------------------
// JSON record parser (K1): one pass, captures fields by path signature
// (PlanView layout: common.h)

// Parses one record (bytes [start,end)); fills fv (all slots must be
// preinitialized to T_MISSING by the caller).  Returns false on invalid
// JSON.  top_type receives the top-level value type.
template <class BS>
DN_HD_INLINE bool parse_record(BS BV, uint32_t start, uint32_t end,
                               const PlanView& P, FV& fv, uint8_t& top_type,
                               uint64_t* sig_lds, bool dot_splits) {
  CursorT<BS> c; c.init(BV, start, end);
  // parent-signature stack in LDS: [depth * BLOCK + tid]
  #define sig_stack_at(d) sig_lds[(d) * BLOCK + DN_TID()]

  uint64_t cont_slot = ~0ull;  // 5 bits/depth: captured slot or 31
  uint64_t is_arr_bits = 0;       // bit d: container at depth d is array
  int depth = 0;                  // container depth (0 = at top value)
  int arr_depth = 0;              // number of array containers on stack
  uint64_t cur_sig = 0;           // path sig for the value being parsed
  bool cur_capture = false;       // does cur_sig match a slot?
  int cur_slot = -1;

  c.skip_ws();
  if (c.eof()) return false;

  // match cur sig against the field table
  auto match_slot = [&](uint64_t sig) -> int {
    if (!((P.sig_bloom >> ((uint32_t)sig & 63u)) & 1ull)) return -1;
    for (int f = 0; f < P.nf; f++)
      if (P.field_sigs[f] == sig) return f;
    return -1;
  };

  // parse the key of an object member (cursor at '"'), extending the
  // parent signature via chained component hashes (plan.path_sig)
  auto parse_key = [&](uint64_t parent, bool root, uint64_t& sig_out) -> bool {
    if (c.eof() || c.next() != '"') return false;
    int r = scan_key_sig(c, root ? FNV_OFFSET : parent, sig_out,
                         dot_splits);
    if (r == 0) return false;
    // skinner: a fields-ROOT key containing a dot is a LITERAL dotted
    // key — addressable by the aggregation lookup (literal-first) but
    // invisible to krill pluck; fold the marker so it captures into
    // the companion slot (plan.py SIG_LIT_MARK)
    if (r == 2 && !root && parent == P.fields_parent_sig)
      sig_out = sig_mix(sig_out ^ SIG_LIT_MARK);
    return true;
  };

  // Main loop: parse values iteratively.
  // expect_value: cursor sits at a value; otherwise we're closing
  // containers / consuming separators.
  bool expect_value = true;
  top_type = T_MISSING;

  while (true) {
    if (expect_value) {
      c.skip_ws();
      if (c.eof()) return false;
      uint8_t b = c.peek();
      uint8_t vtype = T_MISSING;
      uint32_t voff = 0, vlen = 0;
      double vnum = 0.0;

      if (b == '{') {
        uint32_t vstart = c.pos;
        c.pos++;
        // capture the object itself (presence + raw span)
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, T_OBJ, vstart, 0, 0.0);
        if (depth == 0) top_type = T_OBJ;
        if (depth >= MAX_DEPTH) return false;
        c.skip_ws();
        if (!c.eof() && c.peek() == '}') {
          c.pos++;
          vtype = T_OBJ;  // empty object: treat as closed value
          voff = vstart; vlen = c.pos - vstart;
          // fall through to "after value"
        } else {
          // push object frame
          if (depth < SLOT_DEPTH) {
            uint64_t cs = (cur_capture && arr_depth == 0)
                              ? (uint64_t)cur_slot : 31ull;
            cont_slot = (cont_slot & ~(31ull << (5 * depth)))
                        | (cs << (5 * depth));
          }
          if (depth < SIG_DEPTH) sig_stack_at(depth) = cur_sig;
          is_arr_bits &= ~(1ull << depth);
          depth++;
          // parse first key
          uint64_t ksig;
          if (!parse_key(cur_sig, depth == 1, ksig)) return false;
          c.skip_ws();
          if (c.eof() || c.next() != ':') return false;
          cur_sig = ksig;
          cur_slot = (arr_depth == 0) ? match_slot(ksig) : -1;
          cur_capture = cur_slot >= 0;
          continue;  // parse the member value
        }
      } else if (b == '[') {
        uint32_t vstart = c.pos;
        c.pos++;
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, T_ARR, vstart, 0, 0.0);
        if (depth == 0) top_type = T_ARR;
        if (depth >= MAX_DEPTH) return false;
        c.skip_ws();
        if (!c.eof() && c.peek() == ']') {
          c.pos++;
          vtype = T_ARR;
          voff = vstart; vlen = c.pos - vstart;
        } else {
          if (depth < SLOT_DEPTH) {
            uint64_t cs = (cur_capture && arr_depth == 0)
                              ? (uint64_t)cur_slot : 31ull;
            cont_slot = (cont_slot & ~(31ull << (5 * depth)))
                        | (cs << (5 * depth));
          }
          if (depth < SIG_DEPTH) sig_stack_at(depth) = cur_sig;
          is_arr_bits |= (1ull << depth);
          depth++;
          arr_depth++;
          cur_capture = false; cur_slot = -1;
          continue;  // parse first element
        }
      } else if (b == '"') {
        c.pos++;
        if (!scan_string_fast(c, voff, vlen)) return false;
        vtype = T_STR;
      } else if (b == 't') {
        if (c.end - c.pos < 4) return false;
        if (c.byte_at(c.pos+1)!='r'||c.byte_at(c.pos+2)!='u'||c.byte_at(c.pos+3)!='e') return false;
        c.pos += 4; vtype = T_TRUE;
      } else if (b == 'f') {
        if (c.end - c.pos < 5) return false;
        if (c.byte_at(c.pos+1)!='a'||c.byte_at(c.pos+2)!='l'||c.byte_at(c.pos+3)!='s'||c.byte_at(c.pos+4)!='e') return false;
        c.pos += 5; vtype = T_FALSE;
      } else if (b == 'n') {
        if (c.end - c.pos < 4) return false;
        if (c.byte_at(c.pos+1)!='u'||c.byte_at(c.pos+2)!='l'||c.byte_at(c.pos+3)!='l') return false;
        c.pos += 4; vtype = T_NULL;
      } else if (b == '-' || (b >= '0' && b <= '9')) {
        NumOut n = parse_json_number(c);
        if (!n.ok) return false;
        vtype = T_NUM; vnum = n.v;
      } else {
        return false;
      }

      // scalar (or empty-container) value completed
      if (vtype != T_MISSING) {
        if (cur_capture && arr_depth == 0)
          fv.set(cur_slot, vtype, voff, vlen, vnum);
        if (depth == 0) { top_type = (top_type == T_MISSING) ? vtype : top_type; }
      }
      expect_value = false;
      continue;
    }

    // after a value: close containers / separators
    if (depth == 0) {
      c.skip_ws();
      return c.eof();  // trailing garbage -> invalid
    }
    c.skip_ws();
    if (c.eof()) return false;
    uint8_t b = c.next();
    bool in_arr = (is_arr_bits >> (depth - 1)) & 1u;
    if (in_arr) {
      if (b == ',') { expect_value = true; cur_capture = false; cur_slot = -1; continue; }
      if (b == ']') {
        depth--; arr_depth--;
        {
          int cs = (depth < SLOT_DEPTH)
                       ? (int)((cont_slot >> (5 * depth)) & 31ull) : 31;
          if (cs != 31) fv.set_len(cs, c.pos - fv.get_soff(cs));
        }
        // restore parent sig (not needed for captures inside arrays)
        cur_sig = (depth < SIG_DEPTH) ? sig_stack_at(depth) : 0;
        continue;  // still "after value" for the parent
      }
      return false;
    } else {
      if (b == ',') {
        c.skip_ws();
        uint64_t parent = (depth - 1 < SIG_DEPTH) ? sig_stack_at(depth - 1) : 0;
        uint64_t ksig;
        if (!parse_key(parent, depth == 1, ksig)) return false;
        c.skip_ws();
        if (c.eof() || c.next() != ':') return false;
        cur_sig = ksig;
        cur_slot = (arr_depth == 0) ? match_slot(ksig) : -1;
        cur_capture = cur_slot >= 0;
        expect_value = true;
        continue;
      }
      if (b == '}') {
        depth--;
        {
          int cs = (depth < SLOT_DEPTH)
                       ? (int)((cont_slot >> (5 * depth)) & 31ull) : 31;
          if (cs != 31) fv.set_len(cs, c.pos - fv.get_soff(cs));
        }
        cur_sig = (depth < SIG_DEPTH) ? sig_stack_at(depth) : 0;
        continue;
      }
      return false;
    }
  }
}

// -------------------------------------------------------------------
// predicate evaluation (K2): -1 throw (missing field), 0 false, 1 true

template <class BS>
DN_HD_INLINE int eval_leaf(const PlanView& P, BS BV, const FV& fv,
                           int op, int slot, int cidx) {
  uint8_t ft = fv.get_type(slot);
  if (ft == T_MISSING) return -1;  // krill: missing field -> throw

  int ckind = P.const_meta[cidx * 6 + 0];
  uint32_t coff = (uint32_t)P.const_meta[cidx * 6 + 1];
  uint32_t clen = (uint32_t)P.const_meta[cidx * 6 + 2];
  int cdvalid = P.const_meta[cidx * 6 + 3];
  double cdval = P.const_dvals[cidx];

  if (op == OP_EQ || op == OP_NE) {
    bool eq = false;
    if (ft == T_NULL) {
      eq = (ckind == CONST_NULL);
    } else if (ckind == CONST_NULL) {
      eq = false;
    } else if (ft == T_TRUE || ft == T_FALSE || ft == T_NUM) {
      double fnum = (ft == T_NUM) ? fv.get_num(slot) : (ft == T_TRUE ? 1.0 : 0.0);
      if (ckind == CONST_NUM) eq = (fnum == cdval);
      else eq = cdvalid && (fnum == cdval);  // number vs numeric string
    } else if (ft == T_STR) {
      if (ckind == CONST_STR) {
        uint32_t fo = fv.get_soff(slot), fl = fv.get_slen(slot);
        if (fl == clen) {
          eq = true;
          for (uint32_t k = 0; k < fl; k++)
            if (BV.at(fo + k) != P.const_bytes[coff + k]) { eq = false; break; }
        }
        // records may carry the constant in JSON-ESCAPED form: try
        // the canonical escaped rendering too (plan.py ConstPool)
        if (!eq) {
          uint32_t co2 = (uint32_t)P.const_meta[cidx * 6 + 4];
          uint32_t cl2 = (uint32_t)P.const_meta[cidx * 6 + 5];
          if (cl2 != 0 && fl == cl2) {
            eq = true;
            for (uint32_t k = 0; k < fl; k++)
              if (BV.at(fo + k) != P.const_bytes[co2 + k]) { eq = false; break; }
          }
        }
        // NON-canonical escapes in the data (GET, \/, surrogate
        // pairs): unescape-as-you-compare (cold; escaped spans only)
        if (!eq && span_has_backslash(BV, fo, fl))
          eq = unesc_cmp(BV, fo, fl, P.const_bytes + coff, clen) == 0;
      } else {  // string vs number: ToNumber(field)
        double fn = js_to_number(BV, fv.get_soff(slot), fv.get_slen(slot));
        eq = (fn == fn) && (fn == cdval);
      }
    } else {
      eq = false;  // object/array operands never equal scalars
    }
    return (op == OP_EQ) ? (eq ? 1 : 0) : (eq ? 0 : 1);
  }

  // relational
  if (ft == T_STR && ckind == CONST_STR) {
    uint32_t fo = fv.get_soff(slot), fl = fv.get_slen(slot);
    int cmp = 0;
    if (span_has_backslash(BV, fo, fl)) {
      cmp = unesc_cmp(BV, fo, fl, P.const_bytes + coff, clen);
      if (cmp == -2) cmp = 0;  // unreachable: tokenizer validated
    } else {
      uint32_t n = fl < clen ? fl : clen;
      for (uint32_t k = 0; k < n; k++) {
        uint8_t a = BV.at(fo + k), b = P.const_bytes[coff + k];
        if (a != b) { cmp = a < b ? -1 : 1; break; }
      }
      if (cmp == 0) cmp = (fl < clen) ? -1 : (fl > clen ? 1 : 0);
    }
    switch (op) {
      case OP_LT: return cmp < 0;
      case OP_LE: return cmp <= 0;
      case OP_GT: return cmp > 0;
      default:    return cmp >= 0;
    }
  }
  double x, y;
  if (ft == T_NUM) x = fv.get_num(slot);
  else if (ft == T_NULL) x = 0.0;
  else if (ft == T_TRUE) x = 1.0;
  else if (ft == T_FALSE) x = 0.0;
  else if (ft == T_STR) x = js_to_number(BV, fv.get_soff(slot), fv.get_slen(slot));
  else x = __builtin_nan("");  // object/array
  if (ckind == CONST_NUM) y = cdval;
  else if (ckind == CONST_NULL) y = 0.0;
  else y = cdvalid ? cdval : __builtin_nan("");
  if (x != x || y != y) return 0;
  switch (op) {
    case OP_LT: return x < y;
    case OP_LE: return x <= y;
    case OP_GT: return x > y;
    default:    return x >= y;
  }
}

template <class BS>
DN_HD_INLINE int eval_predicate(const PlanView& P, BS BV,
                                const FV& fv, int prog_id) {
  int idx = P.prog_bounds[prog_id * 2 + 0];
  // frame packed into u64: op(1b) | remaining(23b) | end(32b)
  uint64_t stk[PRED_STACK];
  int sp = 0;
  int result;
  while (true) {
    int op = P.prog_nodes[idx * 4 + 0];
    if (op == OP_AND || op == OP_OR) {
      if (sp >= PRED_STACK) return -1;
      stk[sp] = ((uint64_t)(op == OP_OR)
                  | ((uint64_t)P.prog_nodes[idx * 4 + 1] << 1)
                  | ((uint64_t)P.prog_nodes[idx * 4 + 3] << 32));
      sp++;
      idx++;
      continue;
    }
    if (op == OP_TRUE) {
      result = 1;
      idx = P.prog_nodes[idx * 4 + 3];
    } else {
      result = eval_leaf(P, BV, fv, op,
                         P.prog_nodes[idx * 4 + 1],
                         P.prog_nodes[idx * 4 + 2]);
      idx = P.prog_nodes[idx * 4 + 3];
    }
    // unwind (short-circuit exactly like sequential evaluation)
    while (sp > 0) {
      if (result == -1) return -1;  // throw propagates
      uint64_t f = stk[sp - 1];
      bool is_or = f & 1;
      uint32_t remaining = (uint32_t)(f >> 1) & 0x7FFFFF;
      bool sc = (!is_or && result == 0) || (is_or && result == 1);
      remaining--;
      if (sc || remaining == 0) {
        idx = (int)(f >> 32);
        sp--;
      } else {
        stk[sp - 1] = (f & 0xFFFFFFFF00000001ull)
                      | ((uint64_t)remaining << 1);
        break;  // evaluate next child at idx
      }
    }
    if (sp == 0) return result;
  }
}

}  // namespace dn
