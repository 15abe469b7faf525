// rdf_capi_program.inc — the program path: an rdf_expr_node tree compiled to accumulator-machine bytecode, matched against the
// catalogs of specialised kernels (rdf_spec.hip, rdf_spec_shapes.hip, rdf_gspec.hip, the run-time compiler of rdf_jit.cpp) and run
// as ONE fused kernel over a chunk list or a frame; textually included by rdf_capi.cpp behind rdf_frame and frame_tiles /
// frame_col_tab (it uses that file's per-thread context, arena, staging helpers and table builder).  Every scalar kernel,
// aggregate, predicate, rdf_pipeline* and rdf_group_pipeline* entry point and every slab of the streamed batch loop comes through.
//
//   Compiler, build_*_plan        the bytecode; the canonical signatures the catalogs are looked up by
//   run_program                   the driver over the phases below, one ProgramRun on its stack:
//     program_check / _compile      arguments, dtypes, batch lengths; the program and the outputs it implies
//     program_empty                 no rows: the answers (and, in rdf_pipeline_dist, the collective an empty shard still enters)
//     program_stage                 inputs and outputs in HBM, the interpreter's tiles and grid, device scratch
//     eval_tables                   the interpreter's chunk tables — only when it (or the grouped sink) runs
//     spec_choose / spec_tables     catalog -> shape catalog -> run-time compiled; its tables, grid and tile walk
//     run_group / run_agg / run_store   launch and delivery per sink
//   run_program_any               chunk lists: streamed in slabs (rdf_capi_stream.inc) or one run_program
//
// The launch policy itself (blocks per CU, tile walk, LDS copies) is rdf_program_plan.h, with the measurements behind it.

namespace {

// ------------------------------------------------------------------------------------------------
// expression compiler: rdf_expr_node tree -> accumulator-machine bytecode

bool op_is_arith(int op) { return op >= RDF_OP_ADD && op <= RDF_OP_DIV; }
bool op_is_fbinary(int op) { return op >= RDF_OP_ATAN2 && op <= RDF_OP_LOG; }
bool op_is_unary_math(int op) { return (op >= RDF_OP_ABS && op <= RDF_OP_TANH) || (op >= RDF_OP_COT && op <= RDF_OP_CSC); }
bool op_is_cmp(int op) { return op >= RDF_OP_GT && op <= RDF_OP_LE; }
bool op_is_hour(int op) { return op >= RDF_OP_HOUR_S && op <= RDF_OP_HOUR_DAY; }
bool op_is_binary(int op) { return op_is_arith(op) || op_is_fbinary(op) || op_is_cmp(op) || op == RDF_OP_AND || op == RDF_OP_OR; }
bool op_is_heavy(int op) {
    if (op_is_fbinary(op)) return true;
    if (!op_is_unary_math(op)) return false;
    switch (op) {
        case RDF_OP_ABS: case RDF_OP_CEIL: case RDF_OP_FLOOR: case RDF_OP_ROUND: case RDF_OP_SQRT:
        case RDF_OP_DEGREES: case RDF_OP_RADIANS: return false;
        default: return true;
    }
}

struct Compiler {
    const rdf_expr_node* nodes;
    int nnodes;
    const int* col_dtype;
    int ncols;
    std::vector<Instr> code;
    std::vector<int> memo;
    int tmp_used = 0, tmp_max = 0;
    bool heavy = false, intdiv = false;
    bool lossy_cast = false;   // the program holds a cast that can turn a valid value into NULL (arrow::compute::cast: None -> NULL)
    rdf_status st = RDF_OK;
    int feat() const { return heavy ? 2 : intdiv ? 1 : 0; }

    Compiler(const rdf_expr_node* n, int nn, const int* cd, int nc) : nodes(n), nnodes(nn), col_dtype(cd), ncols(nc), memo((size_t)(nn > 0 ? nn : 0), -2) {}

    int bad(rdf_status s, const char* fmt, ...) {
        if (st == RDF_OK) {
            char buf[256];
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, sizeof buf, fmt, ap);
            va_end(ap);
            st = fail(s, "%s", buf);
        }
        return -1;
    }

    // result dtype of node idx (or -1 on error)
    int infer(int idx, int depth = 0) {
        if (idx < 0 || idx >= nnodes) return bad(RDF_INVALID_ARGUMENT, "bad node index %d", idx);
        if (depth > 64) return bad(RDF_INVALID_ARGUMENT, "expression too deep");
        if (memo[(size_t)idx] != -2) return memo[(size_t)idx];
        const rdf_expr_node& nd = nodes[idx];
        int r = -1;
        if (nd.kind == RDF_NODE_COLUMN) {
            if (nd.column < 0 || nd.column >= ncols) r = bad(RDF_COMPUTE_ERROR, "Cannot find column %d", nd.column);
            else r = col_dtype[nd.column];
        } else if (nd.kind == RDF_NODE_SCALAR) {
            if (nd.dtype == RDF_NULLTYPE) r = RDF_BOOL;
            else if (is_numeric(nd.dtype) || nd.dtype == RDF_BOOL) r = nd.dtype;
            else r = bad(RDF_INVALID_ARGUMENT, "unsupported scalar type %d", nd.dtype);
        } else if (nd.kind == RDF_NODE_OP) {
            const int op = nd.op;
            const int l = infer(nd.lhs, depth + 1);
            if (l < 0) return memo[(size_t)idx] = -1;
            if (op_is_binary(op)) {
                const int rr = infer(nd.rhs, depth + 1);
                if (rr < 0) return memo[(size_t)idx] = -1;
                if (op_is_arith(op) || op_is_fbinary(op)) {
                    if (l != rr) r = bad(RDF_INVALID_ARGUMENT, "binary op %d: operand types differ (%d vs %d); insert a Cast", op, l, rr);
                    else if (!is_numeric(l)) r = bad(RDF_INVALID_ARGUMENT, "binary op %d: numeric type required", op);
                    else if (op_is_fbinary(op) && !is_float(l)) r = bad(RDF_INVALID_ARGUMENT, "math_op: float type required");
                    else r = l;
                } else r = RDF_BOOL;  // comparisons, and, or
            } else if (op_is_unary_math(op)) {
                if (op == RDF_OP_ABS) {
                    if (!(is_float(l) || is_signed_int(l))) r = bad(RDF_INVALID_ARGUMENT, "abs: signed numeric type required");
                    else r = l;
                } else if (!is_float(l)) r = bad(RDF_INVALID_ARGUMENT, "float type required");
                else r = l;
            } else if (op_is_hour(op)) {
                if (l != RDF_I32 && l != RDF_I64) r = bad(RDF_INVALID_ARGUMENT, "hour: Int32 / Int64 temporal storage required");
                else r = l;
            } else if (op == RDF_OP_CAST) {
                if (!(is_numeric(nd.dtype) || nd.dtype == RDF_BOOL)) r = bad(RDF_INVALID_ARGUMENT, "cast: unsupported type");
                else r = nd.dtype;
            } else if (op == RDF_OP_NOT) r = RDF_BOOL;
            else r = bad(RDF_INVALID_ARGUMENT, "unsupported op %d", op);
        } else r = bad(RDF_INVALID_ARGUMENT, "bad node kind %d", nd.kind);
        return memo[(size_t)idx] = r;
    }

    bool is_leaf(int idx) const { return nodes[idx].kind != RDF_NODE_OP; }

    void push(Instr in) {
        if ((int)code.size() >= kMaxCode) { bad(RDF_INVALID_ARGUMENT, "expression too long (more than %d steps)", kMaxCode); return; }
        code.push_back(in);
    }
    static Instr mk(uint8_t bc) {
        Instr in;
        memset(&in, 0, sizeof in);
        in.bc = bc;
        return in;
    }

    // literal payload converted on the host into domain `dom`
    uint64_t imm_for(const rdf_expr_node& nd, int dom) {
        const int lt = nd.dtype == RDF_NULLTYPE ? RDF_BOOL : nd.dtype;
        const bool flit = is_float(lt);
        const double f = lt == RDF_F32 ? (double)(float)nd.f64 : nd.f64;
        const uint64_t iv = nd.dtype == RDF_NULLTYPE ? 0 : (lt == RDF_BOOL ? (uint64_t)(nd.i64 != 0) : h_normalize_int(lt, (uint64_t)nd.i64));
        if (dom == RDF_BOOL) return flit ? (uint64_t)(f != 0.0) : (uint64_t)(iv != 0);
        if (dom == RDF_F64) {
            double d = flit ? f : (is_signed_int(lt) ? (double)(int64_t)iv : (double)iv);
            uint64_t u; memcpy(&u, &d, 8); return u;
        }
        if (dom == RDF_F32) {
            float d = flit ? (float)f : (is_signed_int(lt) ? (float)(int64_t)iv : (float)iv);
            uint32_t u; memcpy(&u, &d, 4); return u;
        }
        if (flit) {
            if (f != f) return 0;
            if (is_signed_int(dom)) {
                double lo = dom == RDF_I8 ? -128.0 : dom == RDF_I16 ? -32768.0 : dom == RDF_I32 ? -2147483648.0 : -9223372036854775808.0;
                double hi = dom == RDF_I8 ? 127.0 : dom == RDF_I16 ? 32767.0 : dom == RDF_I32 ? 2147483647.0 : 9223372036854775807.0;
                if (f <= lo) return (uint64_t)(int64_t)lo;
                if (f >= hi) return dom == RDF_I64 ? (uint64_t)INT64_MAX : (uint64_t)(int64_t)hi;
                return (uint64_t)(int64_t)f;
            }
            double hi = dom == RDF_U8 ? 255.0 : dom == RDF_U16 ? 65535.0 : dom == RDF_U32 ? 4294967295.0 : 18446744073709551615.0;
            if (f <= 0.0) return 0;
            if (f >= hi) return dom == RDF_U64 ? ~0ull : (uint64_t)hi;
            return (uint64_t)f;
        }
        return h_normalize_int(dom, iv);
    }

    void operand_fields(Instr& in, int leaf_idx, int dom) {
        const rdf_expr_node& nd = nodes[leaf_idx];
        if (nd.kind == RDF_NODE_COLUMN) {
            in.src_kind = SRC_COL;
            in.src = (uint16_t)nd.column;
            in.src_dtype = (uint8_t)col_dtype[nd.column];
        } else {
            in.src_kind = SRC_IMM;
            in.src_dtype = (uint8_t)dom;
            in.imm = imm_for(nd, dom);
        }
        in.dtype = (uint8_t)dom;
    }
    static bool cast_can_null(int from, int to) {
        if (from == to || to == RDF_BOOL || to == RDF_F32 || to == RDF_F64 || from == RDF_BOOL) return false;
        if (is_float(from)) return true;
        const bool fs = is_signed_int(from), ts = is_signed_int(to);
        const int fb = dtype_size(from), tb = dtype_size(to);
        if (fs == ts) return tb < fb;
        if (fs) return true;
        return tb <= fb;
    }
    void cast_acc(int from, int to) {
        if (from == to) return;
        lossy_cast |= cast_can_null(from, to);
        Instr in = mk(BC_CAST);
        in.src_dtype = (uint8_t)from;
        in.dtype = (uint8_t)to;
        push(in);
    }

    // generate code leaving node idx in the accumulator, in the domain of its inferred dtype
    void gen(int idx) {
        if (st != RDF_OK) return;
        const int dt = infer(idx);
        if (dt < 0) return;
        const rdf_expr_node& nd = nodes[idx];
        if (nd.kind != RDF_NODE_OP) {
            Instr in = mk(BC_LOAD);
            operand_fields(in, idx, dt);
            push(in);
            return;
        }
        const int op = nd.op;
        if (op_is_heavy(op)) heavy = true;
        if ((op == RDF_OP_DIV && !is_float(dt)) || op_is_hour(op)) intdiv = true;
        if (!op_is_binary(op)) {
            gen(nd.lhs);
            const int l = infer(nd.lhs);
            if (op == RDF_OP_CAST) { cast_acc(l, nd.dtype); return; }
            Instr in = mk(BC_UN);
            in.op = (uint8_t)op;
            if (op == RDF_OP_NOT) { cast_acc(l, RDF_BOOL); in.dtype = RDF_BOOL; }
            else in.dtype = (uint8_t)l;
            push(in);
            return;
        }
        const int l = infer(nd.lhs), r = infer(nd.rhs);
        const int dom = op_is_cmp(op) ? RDF_F64 : (op == RDF_OP_AND || op == RDF_OP_OR) ? RDF_BOOL : l;
        Instr in = mk(BC_BIN);
        in.op = (uint8_t)op;
        if (is_leaf(nd.rhs)) {
            gen(nd.lhs);
            cast_acc(l, dom);
            operand_fields(in, nd.rhs, dom);
        } else if (is_leaf(nd.lhs)) {
            gen(nd.rhs);
            cast_acc(r, dom);
            operand_fields(in, nd.lhs, dom);
            in.swapped = 1;
        } else {
            gen(nd.rhs);
            cast_acc(r, dom);
            if (tmp_used >= kMaxTmp) { bad(RDF_INVALID_ARGUMENT, "expression needs more than %d temporaries", kMaxTmp); return; }
            const int slot = tmp_used++;
            if (tmp_used > tmp_max) tmp_max = tmp_used;
            Instr stt = mk(BC_STORE_TMP);
            stt.src = (uint16_t)slot;
            push(stt);
            gen(nd.lhs);
            cast_acc(l, dom);
            in.src_kind = SRC_TMP;
            in.src = (uint16_t)slot;
            in.src_dtype = (uint8_t)dom;
            in.dtype = (uint8_t)dom;
            --tmp_used;
        }
        push(in);
    }
};

// ------------------------------------------------------------------------------------------------
// specialised-kernel lookup: canonical signature of a program (same grammar as rdf_spec.hip's sig())

struct SpecPlan {
    std::string sig;
    int col_map[kGSpecCols];      // canonical column -> program column
    int ncols = 0;
    uint64_t imm[kGSpecImm];
    char imm_tag[kGSpecImm];
    int nimm = 0;
    int width = 0;       // element width of the columns (gspec: of the first one); spec_kernel with `widest`: the program's widest element
    bool widest = false;
    bool ok = true;
    // spec_kernel: 4 columns of one width, 4 literals.  gspec_kernel (grouped sink): 8 columns of any widths,
    // 8 literals, equal literals share one slot
    int max_cols = 4, max_imm = 4;
    bool mixed = false, dedup = false;
};

char spec_tag(int dt) {
    switch (dt) { case RDF_F64: return 'd'; case RDF_I64: return 'l'; case RDF_U64: return 'u'; case RDF_F32: return 'f';
                  case RDF_I32: return 'i'; case RDF_U32: return 'j'; case RDF_BOOL: return 'b';
                  case RDF_I8: return 'a'; case RDF_U8: return 'h'; case RDF_I16: return 's'; case RDF_U16: return 't'; default: return 0; }
}

struct SpecSigBuilder {
    Compiler& cc;
    SpecPlan& sp;
    SpecSigBuilder(Compiler& c, SpecPlan& s) : cc(c), sp(s) {}

    std::string leaf(int idx, int dom) {
        const rdf_expr_node& nd = cc.nodes[idx];
        if (nd.kind == RDF_NODE_COLUMN) {
            const int dt = cc.col_dtype[nd.column];
            if (!spec_tag(dt) || dt == RDF_BOOL) { sp.ok = false; return "?"; }
            if (sp.width == 0 || sp.widest) sp.width = std::max(sp.width, dtype_size(dt));   // spec_kernel: the widest element decides the row layout
            else if (sp.width != dtype_size(dt) && !sp.mixed) { sp.ok = false; return "?"; }  // one width per program
            int id = -1;
            for (int i = 0; i < sp.ncols; ++i) if (sp.col_map[i] == nd.column) id = i;
            if (id < 0) {
                if (sp.ncols >= sp.max_cols) { sp.ok = false; return "?"; }
                id = sp.ncols;
                sp.col_map[sp.ncols++] = nd.column;
            }
            return std::string("c") + char('0' + id) + spec_tag(dt);
        }
        // scalar: payload converted to `dom`
        if (!spec_tag(dom) || dom == RDF_BOOL) { sp.ok = false; return "?"; }
        if (nd.dtype == RDF_NULLTYPE) { sp.ok = false; return "?"; }
        const uint64_t bits = cc.imm_for(nd, dom);
        int id = -1;
        if (sp.dedup)
            for (int i = 0; i < sp.nimm; ++i) if (sp.imm[i] == bits && sp.imm_tag[i] == spec_tag(dom)) id = i;
        if (id < 0) {
            if (sp.nimm >= sp.max_imm) { sp.ok = false; return "?"; }
            id = sp.nimm;
            sp.imm_tag[sp.nimm] = spec_tag(dom);
            sp.imm[sp.nimm++] = bits;
        }
        return std::string("k") + char('0' + id) + spec_tag(dom);
    }

    std::string node(int idx, int dom_for_scalar) {
        if (!sp.ok) return "?";
        const rdf_expr_node& nd = cc.nodes[idx];
        if (nd.kind != RDF_NODE_OP) return leaf(idx, dom_for_scalar);
        const int op = nd.op;
        if (op_is_binary(op)) {
            int l = nd.lhs, r = nd.rhs, o = op;
            const int lt = cc.infer(l), rt = cc.infer(r);
            int dom = op_is_cmp(op) ? RDF_F64 : lt;
            if (op_is_cmp(op) && cc.nodes[l].kind == RDF_NODE_SCALAR && cc.nodes[r].kind != RDF_NODE_SCALAR) {
                std::swap(l, r);  // c CMP x  ==  x CMP' c
                o = op == RDF_OP_GT ? RDF_OP_LT : op == RDF_OP_GE ? RDF_OP_LE : op == RDF_OP_LT ? RDF_OP_GT : op == RDF_OP_LE ? RDF_OP_GE : op;
            }
            (void)rt;
            const std::string a = node(l, dom), b = node(r, dom);
            return "(" + std::to_string(o) + " " + a + " " + b + ")";
        }
        if (op == RDF_OP_CAST) {
            const int from = cc.infer(nd.lhs);
            if (from == nd.dtype) return node(nd.lhs, dom_for_scalar);
            if (!spec_tag(nd.dtype) || nd.dtype == RDF_BOOL) { sp.ok = false; return "?"; }
            return "{" + std::to_string(nd.dtype) + " " + node(nd.lhs, from) + "}";
        }
        return "[" + std::to_string(op) + " " + node(nd.lhs, cc.infer(nd.lhs)) + "]";
    }
};

// Builds the plan; returns true when a specialised kernel exists for this program.
bool build_spec_plan(Compiler& cc, int filter_root, int nvalues, const int* value_roots, int sink, SpecPlan& sp) {
    if (nvalues > 2 || (sink == RDF_SINK_STORE && nvalues != 1)) return false;
    sp.widest = true;
    sp.max_cols = kSpecCols; sp.max_imm = kSpecImm;   // (the catalogs' programs stop at 4 and 4; rdf_jit.cpp compiles up to these)
    SpecSigBuilder b(cc, sp);
    std::string s = "P:";
    s += filter_root >= 0 ? b.node(filter_root, RDF_F64) : std::string("-");
    s += ";V:" + b.node(value_roots[0], cc.infer(value_roots[0]));
    s += ";" + (nvalues > 1 ? b.node(value_roots[1], cc.infer(value_roots[1])) : std::string("-"));
    s += ";S:" + std::to_string(sink == RDF_SINK_AGG ? SINK_AGG : SINK_STORE);
    if (!sp.ok) return false;
    if (sink == RDF_SINK_STORE && cc.infer(value_roots[0]) != RDF_BOOL) sp.width = std::max(sp.width, dtype_size(cc.infer(value_roots[0])));
    sp.sig = s;
    return spec_available(s.c_str()) || (g_ctx.opt_jit && jit_find(s.c_str()) != nullptr);   // in the catalog, or compiled earlier in this process (rdf_jit.cpp)
}

// Second-level lookup: kernels specialised on the tree SHAPE with runtime operators (rdf_expr.hip.h *RT nodes; the 8- and
// 4-byte numeric types).  Every leaf occurrence gets its own canonical column / literal slot, operator slots are numbered
// in pre-order (predicate first).  Canonical operand order, reached by setting the operator's swap bit: the deeper
// subtree first, a subtree before a leaf, a column before a literal (rdf_spec_kernel.hip.h lists the compiled shapes:
// up to three levels of arithmetic, sin / cos / tan over up to two levels, behind no predicate, x CMP c, or
// x CMP c AND|OR y CMP d).
struct ShapeSigBuilder {
    Compiler& cc;
    SpecPlan& sp;
    int* rt;
    int nslots = 0;
    int width = 0;      // element width of the program's columns (one width per program)
    int pred_dt = -1;
    ShapeSigBuilder(Compiler& c, SpecPlan& s, int* r) : cc(c), sp(s), rt(r) {}
    bool is_scalar(int idx) const { return cc.nodes[idx].kind == RDF_NODE_SCALAR; }
    bool is_column(int idx) const { return cc.nodes[idx].kind == RDF_NODE_COLUMN; }
    static bool shape_dtype(int dt) { return dt == RDF_F64 || dt == RDF_I64 || dt == RDF_U64 || dt == RDF_F32 || dt == RDF_I32 || dt == RDF_U32 || dt == RDF_I16 || dt == RDF_U16 || dt == RDF_I8 || dt == RDF_U8; }
    int strip(int idx) {   // skip no-op casts
        while (cc.nodes[idx].kind == RDF_NODE_OP && cc.nodes[idx].op == RDF_OP_CAST && cc.infer(cc.nodes[idx].lhs) == cc.nodes[idx].dtype) idx = cc.nodes[idx].lhs;
        return idx;
    }
    int depth(int idx) {   // levels of operators under (and including) idx; anything the shapes do not hold counts as too deep
        idx = strip(idx);
        const rdf_expr_node& nd = cc.nodes[idx];
        if (nd.kind != RDF_NODE_OP) return 0;
        if (nd.op == RDF_OP_CAST && is_column(strip(nd.lhs))) return 0;   // a cast column is a leaf (the plan builders' cast of an operand)
        if (nd.op == RDF_OP_SIN || nd.op == RDF_OP_COS || nd.op == RDF_OP_TAN) return 1 + depth(nd.lhs);
        if (nd.op >= RDF_OP_ADD && nd.op <= RDF_OP_DIV) return 1 + std::max(depth(nd.lhs), depth(nd.rhs));
        return 100;
    }
    // a leaf in domain `dom`: a column of exactly that dtype, or a literal converted to it
    std::string leaf(int idx, int dom) {
        const rdf_expr_node& nd = cc.nodes[idx];
        const char tag = spec_tag(dom);
        if (nd.kind == RDF_NODE_COLUMN) {
            if (cc.col_dtype[nd.column] != dom || sp.ncols >= 4) { sp.ok = false; return "?"; }
            width = std::max(width, dtype_size(dom));   // the program's widest element; narrower columns are read with narrower vectors
            sp.col_map[sp.ncols] = nd.column;
            return std::string("c") + char('0' + sp.ncols++) + tag;
        }
        if (nd.dtype == RDF_NULLTYPE || sp.nimm >= 4) { sp.ok = false; return "?"; }
        sp.imm[sp.nimm] = cc.imm_for(nd, dom);
        return std::string("k") + char('0' + sp.nimm++) + tag;
    }
    std::string node(int idx, int dom) {
        if (!sp.ok) return "?";
        idx = strip(idx);
        const rdf_expr_node& nd = cc.nodes[idx];
        if (nd.kind != RDF_NODE_OP) return leaf(idx, dom);
        if (nslots >= 8) { sp.ok = false; return "?"; }
        const int op = nd.op;
        if (op == RDF_OP_CAST) {   // cast(column) to the domain's type: a leaf that keeps its own dtype and width in memory
            const int child = strip(nd.lhs);
            if (!is_column(child) || nd.dtype != dom) { sp.ok = false; return "?"; }
            const int from = cc.col_dtype[cc.nodes[child].column];
            if (!shape_dtype(from) || from == dom) { sp.ok = false; return "?"; }
            return "{" + std::to_string(dom) + " " + leaf(child, from) + "}";
        }
        if (op == RDF_OP_SIN || op == RDF_OP_COS || op == RDF_OP_TAN) {
            if (!(dom == RDF_F64 || dom == RDF_F32) || cc.infer(nd.lhs) != dom) { sp.ok = false; return "?"; }
            const int slot = nslots++;
            rt[slot] = op;
            return "[T" + std::to_string(slot) + " " + node(nd.lhs, dom) + "]";
        }
        const bool arith = op >= RDF_OP_ADD && op <= RDF_OP_DIV, cmp = op_is_cmp(op), logic = op == RDF_OP_AND || op == RDF_OP_OR;
        if (!(arith || cmp || logic)) { sp.ok = false; return "?"; }
        int l = strip(nd.lhs), r = strip(nd.rhs);
        if (arith && (cc.infer(idx) != dom || cc.infer(l) != dom || cc.infer(r) != dom)) { sp.ok = false; return "?"; }
        if (cmp && !((is_column(l) && is_scalar(r)) || (is_scalar(l) && is_column(r)))) { sp.ok = false; return "?"; }
        bool swap = false;
        if (!logic) {
            const int dl = depth(l), dr = depth(r);
            if (is_scalar(l) && is_scalar(r)) { sp.ok = false; return "?"; }
            if (dl < dr || (dl == 0 && dr == 0 && is_scalar(l) && is_column(r))) swap = true;
        }
        const int slot = nslots++;
        if (swap && cmp) {          // x CMP c with the literal first: the mirrored operator, operands in canonical order
            const int m = op == RDF_OP_GT ? RDF_OP_LT : op == RDF_OP_GE ? RDF_OP_LE : op == RDF_OP_LT ? RDF_OP_GT : op == RDF_OP_LE ? RDF_OP_GE : op;
            rt[slot] = m;
        } else if (swap && (op == RDF_OP_ADD || op == RDF_OP_MUL)) {
            rt[slot] = op;          // commutative (IEEE addition / multiplication and the wrapping integer ones): no swap needed
        } else {
            rt[slot] = op | (swap ? 0x100 : 0);
        }
        if (swap) std::swap(l, r);
        std::string a, b;
        if (cmp) {   // the column keeps its own dtype, the literal is compared in f64 (src/expression.rs:844-845)
            const int cdt = cc.col_dtype[cc.nodes[l].column];
            if (!shape_dtype(cdt)) { sp.ok = false; return "?"; }
            if (pred_dt >= 0 && pred_dt != cdt) { sp.ok = false; return "?"; }
            pred_dt = cdt;
            a = leaf(l, cdt);
            b = leaf(r, RDF_F64);
        } else { a = node(l, dom); b = node(r, dom); }
        return std::string("(") + (arith ? 'A' : cmp ? 'C' : 'G') + std::to_string(slot) + " " + a + " " + b + ")";
    }
};
bool build_shape_plan(Compiler& cc, int filter_root, int nvalues, const int* value_roots, int sink, SpecPlan& sp, int* rt) {
    if (nvalues != 1) return false;
    ShapeSigBuilder b(cc, sp, rt);
    const int vdt = cc.infer(value_roots[0]);
    const int dom = vdt == RDF_BOOL ? RDF_F64 : vdt;   // a predicate as the value (mask output): its columns pick their own dtype
    if (!ShapeSigBuilder::shape_dtype(dom)) return false;
    std::string s = "P:";
    s += filter_root >= 0 ? b.node(filter_root, RDF_F64) : std::string("-");
    s += ";V:" + b.node(value_roots[0], dom) + ";-;S:" + std::to_string(sink == RDF_SINK_AGG ? SINK_AGG : SINK_STORE);
    if (!sp.ok || b.nslots == 0 || b.width == 0) return false;
    sp.width = sink == RDF_SINK_STORE && vdt != RDF_BOOL ? std::max(b.width, dtype_size(dom)) : b.width;   // a stored value counts too
    sp.sig = s;
    return spec_available(s.c_str());
}

// Grouped sink: signature "G<g>;P:<pred|->;K:<group id>;V:<v0>;<v1>;..." for the smallest catalog G >= ngroups.
bool build_gspec_plan(Compiler& cc, int filter_root, int group_root, int ngroups, int nvalues, const int* value_roots, SpecPlan& sp) {
    sp.max_cols = kGSpecCols; sp.max_imm = kGSpecImm; sp.mixed = true; sp.dedup = true;
    SpecSigBuilder b(cc, sp);
    std::string s = ";P:";
    s += filter_root >= 0 ? b.node(filter_root, RDF_F64) : std::string("-");
    s += ";K:" + b.node(group_root, cc.infer(group_root)) + ";V:";
    for (int v = 0; v < nvalues; ++v) s += b.node(value_roots[v], cc.infer(value_roots[v])) + ";";
    if (!sp.ok) return false;
    for (int g : {2, 4, 6, 8}) {
        if (g < ngroups) continue;
        const std::string full = "G" + std::to_string(g) + s;
        if (gspec_available(full.c_str()) || (g_ctx.opt_jit && jit_find(full.c_str()))) { sp.sig = full; return true; }
    }
    if (g_ctx.opt_jit)   // no catalog holds the program: the grouped kernel template compiled for it at run time (rdf_jit.cpp)
        for (int g : {2, 4, 6, 8}) {
            if (g < ngroups) continue;
            const std::string full = "G" + std::to_string(g) + s;
            if (jit_spec_kernel(full.c_str(), g_ctx.opt_jit >= 2)) { sp.sig = full; return true; }
            break;
        }
    return false;
}

// ------------------------------------------------------------------------------------------------
// the fused evaluator driver

struct ProgramSpec {
    const rdf_expr_node* nodes;
    int nnodes;
    int filter_root;
    int nvalues;
    int value_roots[kMaxGroupValues];
    int sink;
    // RDF_SINK_GROUP (internal): rdf_group_pipeline
    int group_root = -1, ngroups = 0;
    rdf_group_result* gout = nullptr;
    int64_t* grows = nullptr;
    bool casts_always_fit = false;   // internal programs whose narrowing cast cannot fail (rdf_hour: 0..23 into Int32): no output bitmap needed for it
    // SINK_STORE into buffers a frame owns (frame-level operators): the outputs' descriptors are a DEVICE table laid out
    // [nvalues * nchunks], 16-byte aligned values / 8-byte aligned bitmaps per chunk, every chunk with room for its batch;
    // no rdf_out list is walked, lengths / null counts are not reported.  frame_out0 = chunk 0's descriptors (nchunks == 1).
    const DevOutChunk* frame_outs = nullptr;
    DevOutChunk frame_out0[kMaxValues] = {};
    int frame_out_dtype[kMaxValues] = {0, 0, 0, 0};
};
constexpr int RDF_SINK_GROUP = 2;

// a kernel compiled at run time could not be launched (it is marked failed): the caller runs the program again, interpreted
const rdf_status kRetryInterpreted = static_cast<rdf_status>(77);

// Which handler of eval_lean_kernel runs each step of an aggregate program, if every step has one (LH_* in rdf_device.h, the
// kernel's header says what it covers): columns of 8-byte types all held in registers, f64 comparisons, f64 / 64-bit integer
// arithmetic, Boolean connectives, i64 / u64 -> f64 casts, the filter, aggregate sinks of 8-byte values.  The indices go into
// bits 1..7 of Instr::swapped of `lean`, a copy — the program eval_kernel would run is not touched.
bool lean_assign(const EvalArgs& ea, EvalArgs& lean, int sink = SINK_AGG) {
    if (ea.ncols < 1 || ea.ncols > kPreCols || ea.nvalues < 1 || ea.nvalues > kMaxValues || ea.ncode < 1) return false;
    auto wide = [](int dt) { return dt == RDF_F64 || dt == RDF_I64 || dt == RDF_U64; };
    for (int c = 0; c < ea.ncols; ++c) if (!wide(ea.col_dtype[c])) return false;
    lean = ea;
    for (int i = 0; i < ea.ncode; ++i) {
        const Instr& in = ea.code[i];
        const bool same = in.src_dtype == in.dtype;
        int h = LH_NONE;
        switch (in.bc) {
            case BC_LOAD:
                if (in.src_kind == SRC_COL && same && wide(in.dtype) && in.src < ea.ncols) h = LH_LOAD;
                else if (in.src_kind == SRC_IMM && same) h = LH_LOAD;   // (the payload is already in the step's domain)
                break;
            case BC_STORE_TMP: h = LH_STORE_TMP; break;
            case BC_FILTER: h = LH_FILTER; break;
            case BC_EMIT: if ((wide(in.dtype) || (sink == SINK_STORE && in.dtype == RDF_BOOL)) && in.src < ea.nvalues) h = LH_EMIT; break;   // (stored: 8-byte values, or a predicate's bitmap)
            case BC_UN: if (in.op == RDF_OP_NOT) h = LH_NOT; break;
            case BC_CAST:
                if (in.dtype == RDF_F64 && in.src_dtype == RDF_I64) h = LH_CAST_I2F;
                else if (in.dtype == RDF_F64 && in.src_dtype == RDF_U64) h = LH_CAST_U2F;
                break;
            case BC_BIN: {
                // (a 64-bit integer column as the operand of an f64 step is converted on the way in)
                if (!same && !(in.src_kind == SRC_COL && in.dtype == RDF_F64 && (in.src_dtype == RDF_I64 || in.src_dtype == RDF_U64))) break;
                if (in.src_kind == SRC_COL && !(in.src < ea.ncols)) break;
                if (in.src_kind != SRC_COL && in.src_kind != SRC_IMM && in.src_kind != SRC_TMP) break;
                const bool sw = in.swapped & 1;
                const int op = in.op;
                if (op >= RDF_OP_GT && op <= RDF_OP_LE) {
                    // acc CMP b; swapped (b CMP acc) is the mirrored comparison of acc with b
                    static const int fwd[6] = {LH_F_GT, LH_F_GE, LH_F_EQ, LH_F_NE, LH_F_LT, LH_F_LE};
                    static const int mir[6] = {LH_F_LT, LH_F_LE, LH_F_EQ, LH_F_NE, LH_F_GT, LH_F_GE};
                    h = (sw ? mir : fwd)[op - RDF_OP_GT];
                } else if (op == RDF_OP_AND) h = LH_AND;
                else if (op == RDF_OP_OR) h = LH_OR;
                else if (in.dtype == RDF_F64) {
                    if (op == RDF_OP_ADD) h = LH_F_ADD;
                    else if (op == RDF_OP_MUL) h = LH_F_MUL;
                    else if (op == RDF_OP_SUB) h = sw ? LH_F_RSUB : LH_F_SUB;
                    else if (op == RDF_OP_DIV) h = sw ? LH_F_RDIV : LH_F_DIV;
                } else if (in.dtype == RDF_I64 || in.dtype == RDF_U64) {
                    if (op == RDF_OP_ADD) h = LH_I_ADD;
                    else if (op == RDF_OP_MUL) h = LH_I_MUL;
                    else if (op == RDF_OP_SUB) h = sw ? LH_I_RSUB : LH_I_SUB;
                }
            } break;
            default: break;
        }
        if (h == LH_NONE) return false;
        lean.code[i].swapped = (uint8_t)((in.swapped & 1) | (h << 1));
    }
    return true;
}

rdf_status launch_agg_pair(const EvalArgs* ea, const FilterAggF64Args* fa, int cmp, int feat, int grid, int nvalues,
                           const int* cls, AggPartial* partials, AggPartial* result, const char* spec_sig = nullptr,
                           const SpecArgs* sa = nullptr) {
    Ctx& c = g_ctx;
    KernelTimer kt;
    if (sa) {
        const bool jit = jit_find(spec_sig) != nullptr;
        c.last_kernel = std::string("spec_kernel<") + spec_sig + ">" + (jit ? " [compiled at run time]" : "");
        const hipError_t le = launch_spec(spec_sig, *sa, grid, c.stream);
        if (le != hipSuccess && jit) { (void)hipGetLastError(); return kRetryInterpreted; }
        if (le != hipSuccess) return fail(RDF_DEVICE_ERROR, "launch_spec: %s", hipGetErrorString(le));
    }
    else if (fa) { c.last_kernel = "filter_agg_f64_kernel"; HIP_TRY(launch_filter_agg_f64(*fa, cmp, grid, c.stream)); }
    else {
        EvalArgs lean;
        if (c.opt_interp_lean && feat == 0 && lean_assign(*ea, lean)) { c.last_kernel = "eval_kernel<AGG, lean>"; HIP_TRY(launch_eval_lean(lean, SINK_AGG, grid, c.stream, c.opt_interp_lean == 2)); }
        else { c.last_kernel = "eval_kernel<AGG>"; HIP_TRY(launch_eval(*ea, SINK_AGG, feat, grid, c.stream)); }
    }
    kt.stop();
    AggFinalArgs f;
    memset(&f, 0, sizeof f);
    f.partials = partials;
    f.result = result;
    f.nblocks = grid;
    f.nvalues = nvalues;
    for (int k = 0; k < nvalues; ++k) f.value_cls[k] = cls[k];
    HIP_TRY(launch_agg_final(f, c.stream));
    return RDF_OK;
}

void fill_agg_result(rdf_agg_result* r, int dt, const AggPartial& p) {
    memset(r, 0, sizeof *r);
    r->dtype = dt;
    r->count = p.cnt;
    r->is_some = p.cnt > 0;
    if (is_float(dt)) {
        double s, a, b;
        memcpy(&s, &p.sum, 8); memcpy(&a, &p.mn, 8); memcpy(&b, &p.mx, 8);
        r->sum_f64 = dt == RDF_F32 ? (double)(float)s : s;
        if (p.cnt > 0) { r->min_f64 = a; r->max_f64 = b; }
    } else {
        r->sum_i64 = (int64_t)h_normalize_int(dt, p.sum);
        if (p.cnt > 0) { r->min_i64 = (int64_t)p.mn; r->max_i64 = (int64_t)p.mx; }
    }
}

// rdf_capi_comm.inc: this rank's device-resident partial aggregates -> all ranks' -> folded on the device -> host (one wait)
rdf_status agg_dist_finish(::rdf_comm& c, const AggPartial* d_result, const uint32_t* d_flags, int nvalues, const int* cls, AggPartial* h_out, uint32_t* h_flags);

// ------------------------------------------------------------------------------------------------
// run_program: one call of the program path, phase by phase

static_assert(kPlanSinkStore == RDF_SINK_STORE && kPlanSinkAgg == RDF_SINK_AGG, "rdf_program_plan.h: sinks of the C API");
static_assert(kPlanTmpSlotBytes == kVPT * kBlock * 8 + kBlock * 4, "rdf_program_plan.h: a TMP slot of eval_kernel's LDS spill area");

// What the phases of one run_program call share; it lives on the driver's stack.
struct ProgramRun {
    // the call
    const ProgramSpec& ps;
    const rdf_array* cols;
    int ncols;
    int64_t nchunks;
    rdf_out* outs;
    rdf_agg_result* aggs;
    rdf_frame* fc;
    bool grouped, frame_store = false;
    int32_t mem = -1;
    DbgTimer dbg;
    // program_check: column dtypes, batch lengths
    int col_dtype[kMaxCols];
    std::vector<int64_t> clen_own;
    const std::vector<int64_t>* clen = nullptr;       // the frame's, or clen_own
    int64_t total_rows = 0;
    // program_compile
    Compiler cc;
    int value_dtype[kMaxGroupValues];
    int cls[kMaxGroupValues] = {0, 0, 0, 0, 0, 0, 0, 0};
    // program_stage: inputs and SINK_STORE outputs in HBM, the interpreter's tiles and grid, device scratch
    size_t pin_off = 0;                               // the pinned staging buffer is taken up to here
    InputStager in;
    const std::vector<DevChunkCol>* in_dev = nullptr; // the frame's, or in.dev
    Region outr;
    std::vector<DevOutChunk> dev_outs;
    std::vector<int> out_val_item, out_vld_item;
    std::vector<int64_t> tile_start;
    const rdf_frame::Tiles* eval_tiles = nullptr;
    int64_t ntiles = 0;
    int grid = 0;                                     // of the kernel that runs: the interpreter's, until spec_tables / run_agg choose another
    size_t n_nc = 0;
    int gwords = 0;
    void* scratch = nullptr;                          // flags | null counts | partials | result
    uint32_t* d_flags = nullptr;
    int64_t* d_nullc = nullptr;
    AggPartial* d_partials = nullptr;
    AggPartial* d_result = nullptr;                   // behind the partials of `grid` blocks
    EvalArgs ea;
    TableBuilder tb;
    // spec_choose / spec_tables: the specialised kernel, if one runs
    bool use_spec = false;
    SpecPlan sp;
    int rt_ops[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SpecArgs sa;
    TableBuilder stb;

    ProgramRun(const ProgramSpec& p, const rdf_array* c, int nc, int64_t nch, rdf_out* o, rdf_agg_result* a, rdf_frame* f)
        : ps(p), cols(c), ncols(nc), nchunks(nch), outs(o), aggs(a), fc(f), grouped(p.sink == RDF_SINK_GROUP), cc(p.nodes, p.nnodes, col_dtype, nc) {}
};

// Argument and sink checks, column dtypes (chunk 0 decides, every chunk must agree: ChunkedArray::from_arrays, src/table.rs:24-40),
// batch lengths (all columns of RecordBatch c have one length).
rdf_status program_check(ProgramRun& r, const char* len_mismatch_msg) {
    const ProgramSpec& ps = r.ps;
    const rdf_array* cols = r.cols;
    const int ncols = r.ncols;
    const int64_t nchunks = r.nchunks;
    rdf_frame* fc = r.fc;
    if (nchunks < 0) return fail(RDF_INVALID_ARGUMENT, "negative chunk count");
    if (ncols < 0 || ncols > kMaxCols) return fail(RDF_INVALID_ARGUMENT, "a fused program reads at most %d columns", kMaxCols);
    if (ps.nvalues < 1 || ps.nvalues > (r.grouped ? kMaxGroupValues : kMaxValues)) return fail(RDF_INVALID_ARGUMENT, "nvalues out of range");
    if (r.grouped) {
        if (ps.ngroups < 1 || (int64_t)(ps.ngroups + 1) * ps.nvalues > RDF_MAX_GROUP_SLOTS)
            return fail(RDF_INVALID_ARGUMENT, "grouped aggregation: (ngroups + 1) * nvalues must be in [2, %d] (large key domains: rdf_groupby_sum)", RDF_MAX_GROUP_SLOTS);
        if (!ps.gout) return fail(RDF_INVALID_ARGUMENT, "null output pointer");
    }
    if (ps.sink == RDF_SINK_STORE && ps.filter_root >= 0)
        return fail(RDF_INVALID_ARGUMENT, "SINK_STORE with a filter: use rdf_predicate + rdf_filter_columns");
    r.mem = fc ? RDF_MEM_DEVICE : -1;
    if (fc) RDF_TRY(frame_host(*fc));     // a frame returned by an operator mirrors its tables on first need
    if (!fc) RDF_TRY(check_mem(cols, (int64_t)ncols * nchunks, &r.mem));
    if (r.mem < 0) r.mem = ps.sink == RDF_SINK_STORE && r.outs && nchunks > 0 ? r.outs[0].mem : RDF_MEM_HOST;
    r.frame_store = ps.sink == RDF_SINK_STORE && ps.frame_outs != nullptr;
    if (r.frame_store && !fc) return fail(RDF_INVALID_ARGUMENT, "frame-owned outputs need a frame");
    if (ps.sink == RDF_SINK_STORE && nchunks > 0 && !r.frame_store) {
        if (!r.outs) return fail(RDF_INVALID_ARGUMENT, "outs is null");
        RDF_TRY(check_out_mem(r.outs, (int64_t)ps.nvalues * nchunks, r.mem));
    }
    if (ps.sink == RDF_SINK_AGG && !r.aggs) return fail(RDF_INVALID_ARGUMENT, "aggs is null");

    if (fc) {
        for (int k = 0; k < ncols; ++k) r.col_dtype[k] = fc->col_dtype[k];
        r.total_rows = fc->total_rows;
        r.clen = &fc->clen;
        return RDF_OK;
    }
    for (int k = 0; k < ncols; ++k) {
        r.col_dtype[k] = nchunks > 0 ? cols[(int64_t)k * nchunks].dtype : RDF_F64;
        if (!(is_numeric(r.col_dtype[k]) || r.col_dtype[k] == RDF_BOOL)) return fail(RDF_INVALID_ARGUMENT, "column %d: unsupported dtype %d", k, r.col_dtype[k]);
        for (int64_t c = 0; c < nchunks; ++c)
            if (cols[(int64_t)k * nchunks + c].dtype != r.col_dtype[k]) return fail(RDF_INVALID_ARGUMENT, "column %d: chunks differ in dtype", k);
    }
    r.clen_own.assign((size_t)nchunks, 0);
    for (int64_t c = 0; c < nchunks; ++c) {
        r.clen_own[(size_t)c] = ncols > 0 ? cols[c].length : 0;
        for (int k = 1; k < ncols; ++k)
            if (cols[(int64_t)k * nchunks + c].length != r.clen_own[(size_t)c]) return fail(RDF_COMPUTE_ERROR, "%s", len_mismatch_msg);
        r.total_rows += r.clen_own[(size_t)c];
    }
    r.clen = &r.clen_own;
    return RDF_OK;
}

// The program's bytecode (filter, group id, values), the values' dtypes and classes; then the SINK_STORE outputs held to them.
rdf_status program_compile(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    Compiler& cc = r.cc;
    if (ps.filter_root >= 0) {
        const int ft = cc.infer(ps.filter_root);
        if (cc.st != RDF_OK) return cc.st;
        if (ft != RDF_BOOL) return fail(RDF_INVALID_ARGUMENT, "predicate root must be boolean");
        cc.gen(ps.filter_root);
        cc.push(Compiler::mk(BC_FILTER));
    }
    if (r.grouped) {
        const int gt = cc.infer(ps.group_root);
        if (cc.st != RDF_OK) return cc.st;
        if (!(gt == RDF_BOOL || (gt >= RDF_I8 && gt <= RDF_U64))) return fail(RDF_INVALID_ARGUMENT, "group id expression must be integer-valued");
        cc.gen(ps.group_root);
        Instr g = Compiler::mk(BC_GROUP);
        g.dtype = (uint8_t)gt;
        cc.push(g);
    }
    for (int v = 0; v < ps.nvalues; ++v) {
        r.value_dtype[v] = cc.infer(ps.value_roots[v]);
        if (cc.st != RDF_OK) return cc.st;
        if (ps.sink != RDF_SINK_STORE && !(is_numeric(r.value_dtype[v]) || r.value_dtype[v] == RDF_BOOL))
            return fail(RDF_INVALID_ARGUMENT, "aggregate of a non-numeric value");
        r.cls[v] = value_class(r.value_dtype[v]);
        cc.gen(ps.value_roots[v]);
        Instr e = Compiler::mk(BC_EMIT);
        e.src = (uint16_t)v;
        e.dtype = (uint8_t)r.value_dtype[v];
        cc.push(e);
    }
    if (cc.st != RDF_OK) return cc.st;
    if (ps.casts_always_fit) cc.lossy_cast = false;

    if (r.frame_store) {
        for (int v = 0; v < ps.nvalues; ++v)
            if (ps.frame_out_dtype[v] != r.value_dtype[v]) return fail(RDF_INVALID_ARGUMENT, "output dtype %d != expression dtype %d", ps.frame_out_dtype[v], r.value_dtype[v]);
    } else if (ps.sink == RDF_SINK_STORE) {
        const std::vector<int64_t>& clen = *r.clen;
        for (int v = 0; v < ps.nvalues; ++v)
            for (int64_t c = 0; c < r.nchunks; ++c) {
                rdf_out& o = r.outs[(int64_t)v * r.nchunks + c];
                if (o.dtype != r.value_dtype[v]) return fail(RDF_INVALID_ARGUMENT, "output dtype %d != expression dtype %d", o.dtype, r.value_dtype[v]);
                if (o.capacity < clen[(size_t)c]) return fail(RDF_MEMORY_ERROR, "output capacity too small");
                bool nullable = cc.lossy_cast;   // a cast to a narrower / differently signed / integer type yields NULL where the value does not fit
                if (r.fc) nullable |= r.fc->chunk_nullable[(size_t)c] != 0;
                else for (int k = 0; k < r.ncols; ++k) nullable |= r.cols[(int64_t)k * r.nchunks + c].validity != nullptr;
                if (nullable && !o.validity) return fail(RDF_INVALID_ARGUMENT, "output validity buffer required");
                if (clen[(size_t)c] > 0 && !o.values) return fail(RDF_INVALID_ARGUMENT, "null output values pointer");
            }
    }
    return RDF_OK;
}

// The flags word a program's kernels leave -> the call's status.  Bit 0: an integer division by zero.  Bit 1: a group id
// outside the table (grouped sink), or another rank's failure (rdf_pipeline_dist, where it goes first: this rank's own bit 0
// would be about partials nobody is going to read).
rdf_status program_flags_status(uint32_t flags, const ProgramSpec& ps) {
    if ((flags & 2u) && ps.sink == RDF_SINK_AGG && g_ctx.agg_comm) return fail(RDF_COMPUTE_ERROR, "pipeline_dist: another rank failed before the combine");
    if (flags & 1u) return fail(RDF_DIVIDE_BY_ZERO, "Divide by zero error");
    if ((flags & 2u) && ps.sink == RDF_SINK_GROUP) return fail(RDF_COMPUTE_ERROR, "group id outside [0, %d)", ps.ngroups);
    return RDF_OK;
}

// The aggregates' way out, from the device-resident folded partials and flags word: flags + aggregates in one D2H — or, in
// rdf_pipeline_dist, all-gathered and folded on the device without visiting this host, one wait for the total.
rdf_status deliver_agg(ProgramRun& r, const AggPartial* d_result, const uint32_t* d_flags) {
    Ctx& ctx = g_ctx;
    const int nvalues = r.ps.nvalues;
    AggPartial hp[kMaxValues];
    uint32_t flags = 0;
    if (ctx.agg_comm) RDF_TRY(agg_dist_finish(*ctx.agg_comm, d_result, d_flags, nvalues, r.cls, hp, &flags));
    else {
        RDF_TRY(pinned_reserve(r.pin_off + 64 + sizeof(AggPartial) * kMaxValues));
        char* pin = ctx.pinned + r.pin_off;
        HIP_TRY(hipMemcpyAsync(pin, d_flags, 16, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipMemcpyAsync(pin + 64, d_result, sizeof(AggPartial) * (size_t)nvalues, hipMemcpyDeviceToHost, ctx.stream));
        HIP_TRY(hipStreamSynchronize(ctx.stream));
        r.dbg.mark("kernel + result");
        memcpy(&flags, pin, 4);
        memcpy(hp, pin + 64, sizeof(AggPartial) * (size_t)nvalues);
    }
    RDF_TRY(program_flags_status(flags, r.ps));
    for (int v = 0; v < nvalues; ++v) fill_agg_result(&r.aggs[v], r.value_dtype[v], hp[v]);
    return RDF_OK;
}

// total_rows == 0: nothing to launch.
rdf_status program_empty(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    if (r.frame_store) return RDF_OK;
    if (ps.sink == RDF_SINK_STORE) {
        for (int64_t i = 0; i < (int64_t)ps.nvalues * r.nchunks; ++i) { r.outs[i].length = 0; r.outs[i].null_count = 0; }
    } else if (r.grouped) {
        for (int v = 0; v < ps.nvalues; ++v)
            for (int g = 0; g <= ps.ngroups; ++g) {
                rdf_group_result& gr = ps.gout[(size_t)v * (size_t)(ps.ngroups + 1) + (size_t)g];
                memset(&gr, 0, sizeof gr);
                gr.dtype = r.value_dtype[v];
            }
        if (ps.grows) memset(ps.grows, 0, sizeof(int64_t) * (size_t)(ps.ngroups + 1));
    } else if (g_ctx.agg_comm) {
        // rdf_pipeline_dist over an EMPTY shard: the other ranks are about to enter the all-gathers of agg_dist_finish, so this
        // one must too (returning its local zeros left them in the collective until the watchdog aborted the communicator).
        // Its contribution is the fold's identity, built on the host and handed over like a kernel's partials.
        RDF_TRY(ensure_ready());
        Ctx& cx = g_ctx;
        arena_begin();
        void* scr = nullptr;
        const size_t pb = sizeof(AggPartial) * (size_t)ps.nvalues;
        RDF_TRY(arena_alloc(64 + pb, &scr));
        RDF_TRY(pinned_reserve(64 + pb));
        memset(cx.pinned, 0, 64 + pb);
        for (int v = 0; v < ps.nvalues; ++v) {
            AggPartial id;
            memset(&id, 0, sizeof id);
            if (r.cls[v] == CLS_F64) id.mn = id.mx = 0x7FF8000000000000ull;                     // (agg_init, rdf_common.hip.h)
            else if (r.cls[v] == CLS_SIGNED) { id.mn = (uint64_t)INT64_MAX; id.mx = (uint64_t)INT64_MIN; }
            else { id.mn = ~0ull; id.mx = 0; }
            memcpy(cx.pinned + 64 + sizeof(AggPartial) * (size_t)v, &id, sizeof id);
        }
        HIP_TRY(hipMemcpyAsync(scr, cx.pinned, 64 + pb, hipMemcpyHostToDevice, cx.stream));
        return deliver_agg(r, (const AggPartial*)((char*)scr + 64), (const uint32_t*)scr);
    } else {
        for (int v = 0; v < ps.nvalues; ++v) { memset(&r.aggs[v], 0, sizeof r.aggs[v]); r.aggs[v].dtype = r.value_dtype[v]; }
    }
    return RDF_OK;
}

// Inputs staged (or the frame's descriptors taken), the SINK_STORE outputs laid out, the interpreter's tiles and grid, the
// device scratch, EvalArgs without its chunk tables.
rdf_status program_stage(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    const int64_t nchunks = r.nchunks;
    const int ncols = r.ncols;
    rdf_frame* fc = r.fc;
    RDF_TRY(ensure_ready());
    Ctx& ctx = g_ctx;
    arena_begin();
    size_t pin_used = 0;
    if (!fc) {
        r.in.arrays.reserve((size_t)ncols * (size_t)nchunks);
        r.in.plans.reserve((size_t)ncols * (size_t)nchunks);
        for (int64_t i = 0; i < (int64_t)ncols * nchunks; ++i) r.in.add(&r.cols[i]);
        RDF_TRY(r.in.finish(r.pin_off, &pin_used));
        r.pin_off += (pin_used + 255) & ~(size_t)255;
    }
    r.in_dev = fc ? &fc->dev : &r.in.dev;
    r.dbg.mark("stage inputs");

    // outputs (SINK_STORE)
    const std::vector<int64_t>& clen = *r.clen;
    std::vector<DevOutChunk>& dev_outs = r.dev_outs;
    if (r.frame_store) {   // descriptors live on the device; chunk 0's are mirrored for the one-chunk kernels
        if (nchunks == 1) { dev_outs.resize((size_t)ps.nvalues); for (int v = 0; v < ps.nvalues; ++v) dev_outs[(size_t)v] = ps.frame_out0[v]; }
    } else if (ps.sink == RDF_SINK_STORE) {
        dev_outs.resize((size_t)ps.nvalues * nchunks);
        if (r.mem == RDF_MEM_HOST) {
            r.out_val_item.assign(dev_outs.size(), -1);
            r.out_vld_item.assign(dev_outs.size(), -1);
            for (int v = 0; v < ps.nvalues; ++v)
                for (int64_t c = 0; c < nchunks; ++c) {
                    const size_t i = (size_t)((int64_t)v * nchunks + c);
                    const int64_t n = clen[(size_t)c];
                    if (n == 0) continue;
                    const size_t vb = r.value_dtype[v] == RDF_BOOL ? (size_t)((n + 7) / 8) : (size_t)n * (size_t)dtype_size(r.value_dtype[v]);
                    r.out_val_item[i] = r.outr.add(r.outs[i].values, vb);
                    if (r.outs[i].validity) r.out_vld_item[i] = r.outr.add(r.outs[i].validity, (size_t)((n + 7) / 8));
                }
            // word-granular bitmap stores need the items padded to 8 bytes: Region pads every item by >= 16
            RDF_TRY(r.outr.layout());
            for (size_t i = 0; i < dev_outs.size(); ++i) {
                dev_outs[i].values = r.out_val_item[i] >= 0 ? r.outr.ptr(r.out_val_item[i]) : nullptr;
                dev_outs[i].validity = r.out_vld_item[i] >= 0 ? (uint8_t*)r.outr.ptr(r.out_vld_item[i]) : nullptr;
            }
        } else {
            for (size_t i = 0; i < dev_outs.size(); ++i) dev_outs[i] = DevOutChunk{r.outs[i].values, r.outs[i].validity};
        }
    }

    // tiles
    if (fc) { RDF_TRY(frame_tiles(*fc, kEvalTile, &r.eval_tiles)); r.ntiles = r.eval_tiles->ntiles; }
    else {
        r.tile_start.assign((size_t)nchunks + 1, 0);
        r.ntiles = tile_prefix(clen.data(), nchunks, kEvalTile, r.tile_start.data());
    }
    r.grid = (int)(r.ntiles < (int64_t)eval_grid_limit() ? r.ntiles : (int64_t)eval_grid_limit());

    // device scratch: flags | null counts | partials | result
    r.n_nc = ps.sink == RDF_SINK_STORE ? (size_t)ps.nvalues * (size_t)nchunks : 0;
    r.gwords = r.grouped ? group_words(ps.ngroups, ps.nvalues) : 0;
    const size_t scratch_bytes = 16 + r.n_nc * 8 + ((size_t)r.grid + 4) * (r.grouped ? (size_t)r.gwords * 8 : (size_t)ps.nvalues * sizeof(AggPartial));   // + 4: the specialised kernels' grid (wave-granular tiles) may round up past this one
    RDF_TRY(arena_alloc(scratch_bytes, &r.scratch));
    r.d_flags = (uint32_t*)r.scratch;
    r.d_nullc = (int64_t*)((char*)r.scratch + 16);
    r.d_partials = (AggPartial*)((char*)r.scratch + 16 + r.n_nc * 8);
    r.d_result = r.d_partials + (size_t)r.grid * (size_t)ps.nvalues;
    HIP_TRY(hipMemsetAsync(r.scratch, 0, 16 + r.n_nc * 8, ctx.stream));

    EvalArgs& ea = r.ea;
    memset(&ea, 0, sizeof ea);
    ea.nchunks = nchunks;
    ea.ntiles = r.ntiles;
    ea.ncols = ncols;
    ea.nvalues = ps.nvalues;
    ea.ncode = (int)r.cc.code.size();
    ea.ntmp = r.cc.tmp_max;
    ea.flags = r.d_flags;
    ea.out_null_counts = r.d_nullc;
    ea.partials = r.d_partials;
    for (int k = 0; k < ncols; ++k) ea.col_dtype[k] = r.col_dtype[k];
    for (int v = 0; v < ps.nvalues; ++v) ea.value_cls[v] = r.cls[v];
    memcpy(ea.code, r.cc.code.data(), r.cc.code.size() * sizeof(Instr));
    return RDF_OK;
}

// The general evaluator's chunk tables (descriptors, tile prefix, lengths): built only when that kernel (or the grouped
// sink, which shares them) is going to run — for a frame of a million 1024-row batches they are 40 MB of host work
// and upload that a specialised kernel, which carries its own tables, never reads.
rdf_status eval_tables(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    EvalArgs& ea = r.ea;
    TableBuilder& tb = r.tb;
    rdf_frame* fc = r.fc;
    const std::vector<DevChunkCol>& in_dev = *r.in_dev;
    const std::vector<DevOutChunk>& dev_outs = r.dev_outs;
    const std::vector<int64_t>& clen = *r.clen;
    if (r.nchunks == 1) {
        for (int k = 0; k < r.ncols; ++k) ea.inline_cols[k] = in_dev[(size_t)k];
        for (int v = 0; v < ps.nvalues && ps.sink == RDF_SINK_STORE; ++v) ea.inline_outs[v] = dev_outs[(size_t)v];
        ea.inline_len = clen[0];
    } else if (fc && r.frame_store) {
        ea.cols = fc->d_cols;
        ea.chunk_tile_start = r.eval_tiles->d_start;
        ea.chunk_len = fc->d_clen;
        ea.outs = const_cast<DevOutChunk*>(ps.frame_outs);
    } else if (fc) {   // the frame's own tables; only the outputs' descriptors are per call
        ea.cols = fc->d_cols;
        ea.chunk_tile_start = r.eval_tiles->d_start;
        ea.chunk_len = fc->d_clen;
        const size_t o_outs = tb.reserve(sizeof(DevOutChunk) * (dev_outs.size() + 1));
        RDF_TRY(tb.bind(r.pin_off));
        if (!dev_outs.empty()) memcpy(tb.at<char>(o_outs), dev_outs.data(), sizeof(DevOutChunk) * dev_outs.size());
        RDF_TRY(tb.alloc());
        RDF_TRY(tb.upload(r.pin_off));
        r.pin_off += (tb.size + 255) & ~(size_t)255;
        ea.outs = tb.dev_at<DevOutChunk>(o_outs);
    } else {
        const size_t o_cols = tb.reserve(sizeof(DevChunkCol) * in_dev.size());
        const size_t o_ts = tb.reserve(sizeof(int64_t) * r.tile_start.size());
        const size_t o_len = tb.reserve(sizeof(int64_t) * clen.size());
        const size_t o_outs = tb.reserve(sizeof(DevOutChunk) * (dev_outs.size() + 1));
        RDF_TRY(tb.bind(r.pin_off));
        memcpy(tb.at<char>(o_cols), in_dev.data(), sizeof(DevChunkCol) * in_dev.size());
        memcpy(tb.at<char>(o_ts), r.tile_start.data(), sizeof(int64_t) * r.tile_start.size());
        memcpy(tb.at<char>(o_len), clen.data(), sizeof(int64_t) * clen.size());
        if (!dev_outs.empty()) memcpy(tb.at<char>(o_outs), dev_outs.data(), sizeof(DevOutChunk) * dev_outs.size());
        RDF_TRY(tb.alloc());
        RDF_TRY(tb.upload(r.pin_off));
        r.pin_off += (tb.size + 255) & ~(size_t)255;
        ea.cols = tb.dev_at<DevChunkCol>(o_cols);
        ea.chunk_tile_start = tb.dev_at<int64_t>(o_ts);
        ea.chunk_len = tb.dev_at<int64_t>(o_len);
        ea.outs = tb.dev_at<DevOutChunk>(o_outs);
    }
    return RDF_OK;
}

// A specialised straight-line kernel for this program?  The exact shape from the catalog, else a shape-specialised kernel with
// runtime operators, else the kernel template compiled for it at run time; and every column (and output) aligned for its vectors.
void spec_choose(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    Ctx& ctx = g_ctx;
    SpecPlan& sp = r.sp;
    if (!ctx.opt_spec || r.grouped) return;
    bool have_plan = build_spec_plan(r.cc, ps.filter_root, ps.nvalues, ps.value_roots, ps.sink, sp);
    if (!have_plan) {   // exact shape not in the catalog: a shape-specialised kernel with runtime operators?
        sp = SpecPlan();
        have_plan = build_shape_plan(r.cc, ps.filter_root, ps.nvalues, ps.value_roots, ps.sink, sp, r.rt_ops);
    }
    if (!have_plan && ctx.opt_jit) {
        // neither: the same kernel template instantiated for exactly this program at run time (rdf_jit.cpp) — up to 4 columns and
        // 4 literals, any tree over them; a second or so the first time a process meets the shape, then cached
        sp = SpecPlan();
        for (int k = 0; k < 8; ++k) r.rt_ops[k] = 0;
        (void)build_spec_plan(r.cc, ps.filter_root, ps.nvalues, ps.value_roots, ps.sink, sp);
        if (getenv("RDF_DEBUG_JIT")) fprintf(stderr, "[rdf] jit: candidate %s (ok %d)\n", sp.sig.c_str(), (int)sp.ok);
        have_plan = sp.ok && !sp.sig.empty() && jit_spec_kernel(sp.sig.c_str(), ctx.opt_jit >= 2) != nullptr;
    }
    if (!have_plan) return;
    const int64_t nchunks = r.nchunks;
    const std::vector<int64_t>& clen = *r.clen;
    bool ok = true;
    for (int k = 0; k < sp.ncols && ok; ++k) {
        if (r.fc) { ok = r.fc->col_aligned16[sp.col_map[k]]; continue; }
        const int es = dtype_size(r.col_dtype[sp.col_map[k]]);                       // a vector slot of this column: 16 / width of its elements
        const uintptr_t amask = (uintptr_t)(16 / std::max(sp.width, 1)) * (uintptr_t)es - 1;
        for (int64_t c = 0; c < nchunks; ++c) {
            const DevChunkCol& d = (*r.in_dev)[(size_t)((int64_t)sp.col_map[k] * nchunks + c)];
            if (clen[(size_t)c] > 0 && ((uintptr_t)((const char*)d.values + d.offset * es) & amask) != 0) { ok = false; break; }
        }
    }
    if (ps.sink == RDF_SINK_STORE && !r.frame_store)
        for (int64_t c = 0; c < nchunks && ok; ++c)
            if (clen[(size_t)c] > 0 && (((uintptr_t)r.dev_outs[(size_t)c].values & 15) != 0 || ((uintptr_t)r.dev_outs[(size_t)c].validity & 7) != 0)) ok = false;
    r.use_spec = ok;
}

// SpecArgs of the chosen kernel: literals, its own chunk tables (one chunk inline, a frame's cached tables, or a chunk list
// uploaded with the call), the persistent grid and the tile walk (rdf_program_plan.h: spec_walk_plan).
rdf_status spec_tables(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    Ctx& ctx = g_ctx;
    const SpecPlan& sp = r.sp;
    SpecArgs& sa = r.sa;
    TableBuilder& stb = r.stb;
    rdf_frame* fc = r.fc;
    const int64_t nchunks = r.nchunks;
    const std::vector<DevChunkCol>& in_dev = *r.in_dev;
    const std::vector<int64_t>& clen = *r.clen;
    memset(&sa, 0, sizeof sa);
    const int spec_rpb = spec_rows_per_tile(sp.sig.c_str());
    for (int k = 0; k < sp.nimm; ++k) sa.imm[k] = sp.imm[k];
    for (int k = 0; k < 8; ++k) sa.rt[k] = r.rt_ops[k];
    for (int k = 0; k < kSpecCols; ++k) {   // a repeated program column is loaded once
        sa.alias[k] = -1;
        for (int j = 0; j < k && k < sp.ncols; ++j) if (sp.col_map[j] == sp.col_map[k]) { sa.alias[k] = j; break; }
    }
    sa.partials = r.d_partials;
    sa.flags = r.d_flags;
    sa.vec_bitmap = ctx.opt_vec_bitmap ? 1 : 0;
    sa.out_null_count = r.d_nullc;
    sa.nchunks = nchunks;
    std::vector<int64_t> sts;
    const rdf_frame::Tiles* spec_tiles = nullptr;
    if (fc) {
        RDF_TRY(frame_tiles(*fc, spec_rpb, &spec_tiles));
        sa.ntiles = spec_tiles->ntiles;
        sa.tile_inv = spec_tiles->tile_inv;
    } else {
        sts.assign((size_t)nchunks + 1, 0);
        sa.ntiles = tile_prefix(clen.data(), nchunks, spec_rpb, sts.data());
        sa.tile_inv = tile_reciprocal(nchunks, sts[(size_t)nchunks - 1]);
    }
    if (nchunks == 1) {
        for (int k = 0; k < sp.ncols; ++k) sa.cols[k] = in_dev[(size_t)sp.col_map[k]];
        sa.n = clen[0];
        if (ps.sink == RDF_SINK_STORE) sa.out = r.dev_outs[0];
    } else if (fc) {
        DevChunkCol* tab = nullptr;
        RDF_TRY(frame_col_tab(*fc, sp.col_map, sp.ncols, &tab));
        sa.cols_tab = tab;
        sa.chunk_tile_start = spec_tiles->d_start;
        sa.chunk_len = fc->d_clen;
        if (r.frame_store) sa.outs_tab = ps.frame_outs;
        else if (ps.sink == RDF_SINK_STORE) {   // the outputs' descriptors are per call
            const size_t o_o = stb.reserve(sizeof(DevOutChunk) * ((size_t)nchunks + 1));
            RDF_TRY(stb.bind(r.pin_off));
            memcpy(stb.at<char>(o_o), r.dev_outs.data(), sizeof(DevOutChunk) * (size_t)nchunks);
            RDF_TRY(stb.alloc());
            RDF_TRY(stb.upload(r.pin_off));
            r.pin_off += (stb.size + 255) & ~(size_t)255;
            sa.outs_tab = stb.dev_at<DevOutChunk>(o_o);
        }
    } else {
        const size_t o_c = stb.reserve(sizeof(DevChunkCol) * (size_t)(sp.ncols > 0 ? sp.ncols : 1) * (size_t)nchunks);
        const size_t o_t = stb.reserve(sizeof(int64_t) * sts.size());
        const size_t o_l = stb.reserve(sizeof(int64_t) * clen.size());
        const size_t o_o = stb.reserve(sizeof(DevOutChunk) * ((size_t)nchunks + 1));
        RDF_TRY(stb.bind(r.pin_off));
        for (int k = 0; k < sp.ncols; ++k)
            memcpy(stb.at<DevChunkCol>(o_c) + (size_t)k * (size_t)nchunks, in_dev.data() + (size_t)sp.col_map[k] * (size_t)nchunks, sizeof(DevChunkCol) * (size_t)nchunks);
        memcpy(stb.at<char>(o_t), sts.data(), sizeof(int64_t) * sts.size());
        memcpy(stb.at<char>(o_l), clen.data(), sizeof(int64_t) * clen.size());
        if (ps.sink == RDF_SINK_STORE) memcpy(stb.at<char>(o_o), r.dev_outs.data(), sizeof(DevOutChunk) * (size_t)nchunks);
        RDF_TRY(stb.alloc());
        RDF_TRY(stb.upload(r.pin_off));
        r.pin_off += (stb.size + 255) & ~(size_t)255;
        sa.cols_tab = stb.dev_at<DevChunkCol>(o_c);
        sa.chunk_tile_start = stb.dev_at<int64_t>(o_t);
        sa.chunk_len = stb.dev_at<int64_t>(o_l);
        sa.outs_tab = stb.dev_at<DevOutChunk>(o_o);
    }
    SpecWalkIn wi;
    wi.sink = ps.sink;
    wi.heavy = false;
    for (int i = 0; i < ps.nnodes; ++i) wi.heavy |= ps.nodes[i].kind == RDF_NODE_OP && op_is_heavy(ps.nodes[i].op);
    wi.nchunks = nchunks;
    wi.ncols = sp.ncols;
    wi.any_bitmap = false;
    for (int k = 0; k < sp.ncols; ++k) wi.any_bitmap |= fc ? fc->col_nullable[sp.col_map[k]] : in_dev[(size_t)((int64_t)sp.col_map[k] * nchunks)].validity != nullptr;
    wi.ntiles = sa.ntiles;
    wi.grid_limit = eval_grid_limit();
    wi.waves_per_block = kBlock / 64;
    wi.spec_blocks_per_cu = ctx.opt_spec_blocks;
    wi.spec_tile_rot = ctx.opt_spec_tile_rot;
    wi.spec_xcd_swz = ctx.opt_spec_xcd_swz;
    wi.spec_grid_adj = ctx.opt_spec_grid_adj;
    const WalkPlan wp = spec_walk_plan(wi);
    r.grid = wp.grid;
    sa.tile_rot = wp.tile_rot;
    sa.xcd_swz = wp.xcd_swz;
    r.d_result = r.d_partials + (size_t)r.grid * (size_t)ps.nvalues;
    return RDF_OK;
}

// The grouped sink: gspec_kernel where a catalog (or the run-time compiler) holds the program and every column is aligned for
// 2-row vector loads, else the interpreter; group_final folds the blocks' tables; flags + table in one D2H.
rdf_status run_group(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    Ctx& ctx = g_ctx;
    EvalArgs& ea = r.ea;
    const int64_t nchunks = r.nchunks;
    const std::vector<DevChunkCol>& in_dev = *r.in_dev;
    const std::vector<int64_t>& clen = *r.clen;
    const int gwords = r.gwords;
    ea.ngroups = ps.ngroups;
    ea.group_replicas = group_replicas(gwords, r.cc.tmp_max);
    uint64_t* d_gpart = (uint64_t*)r.d_partials;
    uint64_t* d_gres = d_gpart + (size_t)r.grid * (size_t)gwords;
    ea.group_partials = d_gpart;
    SpecPlan gp;
    bool use_gspec = ctx.opt_spec && ps.ngroups <= 8 &&
                     build_gspec_plan(r.cc, ps.filter_root, ps.group_root, ps.ngroups, ps.nvalues, ps.value_roots, gp);
    for (int k = 0; k < gp.ncols && use_gspec; ++k) {
        const int w = dtype_size(r.col_dtype[gp.col_map[k]]);
        for (int64_t c = 0; c < nchunks; ++c) {
            const DevChunkCol& d = in_dev[(size_t)((int64_t)gp.col_map[k] * nchunks + c)];
            if (clen[(size_t)c] > 0 && ((uintptr_t)((const char*)d.values + d.offset * w) & (uintptr_t)(2 * w - 1)) != 0) { use_gspec = false; break; }
        }
    }
    if (use_gspec) {
        GSpecArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.cols_tab = ea.cols; ga.chunk_tile_start = ea.chunk_tile_start; ga.chunk_len = ea.chunk_len;
        ga.nchunks = nchunks; ga.ntiles = r.ntiles; ga.n = clen[0];
        for (int k = 0; k < gp.ncols; ++k) { ga.col_map[k] = gp.col_map[k]; if (nchunks == 1) ga.cols[k] = in_dev[(size_t)gp.col_map[k]]; }
        for (int k = 0; k < gp.nimm; ++k) ga.imm[k] = gp.imm[k];
        ga.group_partials = d_gpart; ga.flags = r.d_flags;
        ga.ngroups = ps.ngroups; ga.nvalues = ps.nvalues; ga.vec_bitmap = ctx.opt_vec_bitmap ? 1 : 0;
        const WalkPlan wp = gspec_walk_plan(r.grid, eval_grid_limit(), ctx.opt_gspec_blocks, ctx.opt_spec_tile_rot, ctx.opt_spec_xcd_swz);
        r.grid = wp.grid;
        ga.xcd_swz = wp.xcd_swz;
        ga.tile_rot = wp.tile_rot;
        KernelTimer kt;
        ctx.last_kernel = "gspec_kernel<" + gp.sig + ">" + (jit_find(gp.sig.c_str()) ? " [compiled at run time]" : "");
        const hipError_t le = launch_gspec(gp.sig.c_str(), ga, r.grid, ctx.stream);
        if (le != hipSuccess && jit_find(gp.sig.c_str()) == nullptr && !gspec_available(gp.sig.c_str())) {     // a run-time kernel that could not be launched (now marked failed)
            (void)hipGetLastError();
            return kRetryInterpreted;
        }
        if (le != hipSuccess) return fail(RDF_DEVICE_ERROR, "launch_gspec: %s", hipGetErrorString(le));
        kt.stop();
    } else {
        KernelTimer kt;
        ctx.last_kernel = "eval_kernel<GROUP>";
        HIP_TRY(launch_eval(ea, SINK_GROUP, r.cc.feat(), r.grid, ctx.stream));
        kt.stop();
    }
    GroupFinalArgs gf;
    memset(&gf, 0, sizeof gf);
    gf.partials = d_gpart; gf.result = d_gres; gf.nblocks = r.grid; gf.words = gwords; gf.ngroups = ps.ngroups; gf.nvalues = ps.nvalues;
    for (int v = 0; v < ps.nvalues; ++v) gf.value_cls[v] = r.cls[v];
    HIP_TRY(launch_group_final(gf, ctx.stream));
    RDF_TRY(pinned_reserve(r.pin_off + 64 + (size_t)gwords * 8));
    char* pin = ctx.pinned + r.pin_off;
    HIP_TRY(hipMemcpyAsync(pin, r.d_flags, 16, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipMemcpyAsync(pin + 64, d_gres, (size_t)gwords * 8, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipStreamSynchronize(ctx.stream));
    uint32_t flags;
    memcpy(&flags, pin, 4);
    RDF_TRY(program_flags_status(flags, ps));
    const uint64_t* w = (const uint64_t*)(pin + 64);
    const int S = ps.ngroups + 1;
    for (int v = 0; v < ps.nvalues; ++v)
        for (int g = 0; g < S; ++g) {
            rdf_group_result& gr = ps.gout[(size_t)v * (size_t)S + (size_t)g];
            memset(&gr, 0, sizeof gr);
            gr.dtype = r.value_dtype[v];
            gr.count = (int64_t)(w[2 * ps.nvalues * S + g] - w[(ps.nvalues + v) * S + g]);
            gr.is_some = gr.count > 0;
            if (is_float(r.value_dtype[v])) memcpy(&gr.sum_f64, &w[v * S + g], 8);
            else gr.sum_i64 = (int64_t)w[v * S + g];
        }
    if (ps.grows) for (int g = 0; g < S; ++g) ps.grows[g] = (int64_t)w[2 * ps.nvalues * S + g];
    return RDF_OK;
}

// filter(x CMP c) -> aggregates of y, both f64, one chunk, the two columns equally placed within 16 bytes: filter_agg_f64_kernel,
// which handles 8-byte-misaligned columns.  Fills `fa` and the comparison (mirrored for c CMP x) when the program is one.
bool fast_filter_match(ProgramRun& r, FilterAggF64Args& fa, int& cmp) {
    const ProgramSpec& ps = r.ps;
    if (!g_ctx.opt_fast_filter || r.nchunks != 1 || ps.nvalues != 1 || ps.filter_root < 0) return false;
    const rdf_expr_node& fr = ps.nodes[ps.filter_root];
    const rdf_expr_node& vr = ps.nodes[ps.value_roots[0]];
    if (!(fr.kind == RDF_NODE_OP && op_is_cmp(fr.op) && vr.kind == RDF_NODE_COLUMN && r.col_dtype[vr.column] == RDF_F64)) return false;
    const rdf_expr_node& L = ps.nodes[fr.lhs];
    const rdf_expr_node& R = ps.nodes[fr.rhs];
    const rdf_expr_node* coln = nullptr;
    const rdf_expr_node* sc = nullptr;
    cmp = fr.op;
    if (L.kind == RDF_NODE_COLUMN && R.kind == RDF_NODE_SCALAR) { coln = &L; sc = &R; }
    else if (L.kind == RDF_NODE_SCALAR && R.kind == RDF_NODE_COLUMN) {
        coln = &R; sc = &L;  // c CMP x  ==  x CMP' c
        cmp = fr.op == RDF_OP_GT ? RDF_OP_LT : fr.op == RDF_OP_GE ? RDF_OP_LE : fr.op == RDF_OP_LT ? RDF_OP_GT : fr.op == RDF_OP_LE ? RDF_OP_GE : fr.op;
    }
    if (!(coln && r.col_dtype[coln->column] == RDF_F64 && sc->dtype != RDF_NULLTYPE && (is_numeric(sc->dtype) || sc->dtype == RDF_BOOL))) return false;
    const DevChunkCol& x = (*r.in_dev)[(size_t)coln->column];
    const DevChunkCol& y = (*r.in_dev)[(size_t)vr.column];
    const uintptr_t xa = (uintptr_t)((const double*)x.values + x.offset), ya = (uintptr_t)((const double*)y.values + y.offset);
    if (!((xa & 7) == 0 && (ya & 7) == 0 && (xa & 15) == (ya & 15))) return false;
    memset(&fa, 0, sizeof fa);
    fa.x = (const double*)x.values; fa.x_validity = x.validity; fa.x_offset = x.offset;
    fa.y = (const double*)y.values; fa.y_validity = y.validity; fa.y_offset = y.offset;
    fa.n = (*r.clen)[0];
    const uint64_t cu = r.cc.imm_for(*sc, RDF_F64);
    memcpy(&fa.c, &cu, 8);
    fa.partials = r.d_partials;
    return true;
}

// The aggregate sink: the specialised kernel, filter_agg_f64_kernel, or the interpreter (lean where it can be), each followed by
// agg_final; then the results' way out.
rdf_status run_agg(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    FilterAggF64Args fa;
    int cmp = 0;
    if (r.use_spec) {
        RDF_TRY(launch_agg_pair(nullptr, nullptr, 0, 0, r.grid, ps.nvalues, r.cls, r.d_partials, r.d_result, r.sp.sig.c_str(), &r.sa));   // (kRetryInterpreted goes up to the driver)
    } else if (fast_filter_match(r, fa, cmp)) {
        const int64_t per_block = (int64_t)kBlock * 4 * 2;  // rows per block iteration
        const int64_t want = ((*r.clen)[0] + per_block - 1) / per_block;
        r.grid = (int)(want < (int64_t)eval_grid_limit() ? want : (int64_t)eval_grid_limit());
        if (r.grid < 1) r.grid = 1;
        // partials/result were sized for the eval grid (>= this grid, since its tiles are smaller)
        r.d_result = r.d_partials + (size_t)r.grid * (size_t)ps.nvalues;
        RDF_TRY(launch_agg_pair(nullptr, &fa, cmp, 0, r.grid, 1, r.cls, r.d_partials, r.d_result));
    } else {
        RDF_TRY(launch_agg_pair(&r.ea, nullptr, 0, r.cc.feat(), r.grid, ps.nvalues, r.cls, r.d_partials, r.d_result));
    }
    return deliver_agg(r, r.d_result, r.d_flags);
}

// SINK_STORE: the specialised kernel or the interpreter (lean where it can be), then the flags, the null counts and — for host
// outputs — the columns on their way back.
rdf_status run_store(ProgramRun& r) {
    const ProgramSpec& ps = r.ps;
    Ctx& ctx = g_ctx;
    const int64_t nchunks = r.nchunks;
    const std::vector<int64_t>& clen = *r.clen;
    {
        KernelTimer kt;
        if (r.use_spec) {
            const bool jit = jit_find(r.sp.sig.c_str()) != nullptr;
            ctx.last_kernel = "spec_kernel<" + r.sp.sig + ">" + (jit ? " [compiled at run time]" : "");
            const hipError_t le = launch_spec(r.sp.sig.c_str(), r.sa, r.grid, ctx.stream);
            if (le != hipSuccess && jit) { (void)hipGetLastError(); return kRetryInterpreted; }   // marked failed: interpreted this time and from now on
            if (le != hipSuccess) return fail(RDF_DEVICE_ERROR, "launch_spec: %s", hipGetErrorString(le));
        }
        else {
            // (the lean kernel adds a tile's NULLs into the low word of the chunk's 64-bit count: chunks of 2^32 rows and more stay on eval_kernel)
            int64_t longest = 0;
            for (int64_t i = 0; i < nchunks; ++i) longest = std::max(longest, clen[(size_t)i]);
            EvalArgs lean;
            if (ctx.opt_interp_lean && r.cc.feat() == 0 && longest < ((int64_t)1 << 32) && lean_assign(r.ea, lean, SINK_STORE)) {
                ctx.last_kernel = "eval_kernel<STORE, lean>";
                HIP_TRY(launch_eval_lean(lean, SINK_STORE, r.grid, ctx.stream, ctx.opt_interp_lean == 2));
            } else { ctx.last_kernel = "eval_kernel<STORE>"; HIP_TRY(launch_eval(r.ea, SINK_STORE, r.cc.feat(), r.grid, ctx.stream)); }
        }
        kt.stop();
    }
    // frame-owned outputs: flags only — lengths are the frame's batch lengths, null counts stay on the device
    const size_t head = r.frame_store ? 16 : 16 + r.n_nc * 8;
    RDF_TRY(pinned_reserve(r.pin_off + 64 + (r.frame_store ? 0 : r.n_nc * 8 + r.outr.small_bytes + 256)));
    char* pin = ctx.pinned + r.pin_off;
    HIP_TRY(hipMemcpyAsync(pin, r.scratch, head, hipMemcpyDeviceToHost, ctx.stream));
    if (!r.frame_store && r.mem == RDF_MEM_HOST) RDF_TRY(r.outr.download(r.pin_off + ((head + 255) & ~(size_t)255)));
    else HIP_TRY(hipStreamSynchronize(ctx.stream));
    uint32_t flags;
    memcpy(&flags, pin, 4);
    RDF_TRY(program_flags_status(flags, ps));
    if (r.frame_store) return RDF_OK;
    for (int v = 0; v < ps.nvalues; ++v)
        for (int64_t c = 0; c < nchunks; ++c) {
            rdf_out& o = r.outs[(int64_t)v * nchunks + c];
            o.length = clen[(size_t)c];
            memcpy(&o.null_count, pin + 16 + 8 * (size_t)((int64_t)v * nchunks + c), 8);
        }
    return RDF_OK;
}

// One program over a chunk list or a frame.  A kernel compiled at run time that cannot be launched is marked failed, and the
// whole call starts again from the top: the catalogs or the interpreter answer this time and from now on.
rdf_status run_program(const ProgramSpec& ps, const rdf_array* cols, int ncols, int64_t nchunks, rdf_out* outs,
                       rdf_agg_result* aggs, const char* len_mismatch_msg, rdf_frame* fc = nullptr) {
    for (;;) {
        ProgramRun r(ps, cols, ncols, nchunks, outs, aggs, fc);
        RDF_TRY(program_check(r, len_mismatch_msg));
        r.dbg.mark("validate");
        RDF_TRY(program_compile(r));
        if (r.total_rows == 0) return program_empty(r);
        RDF_TRY(program_stage(r));
        if (r.grouped) RDF_TRY(eval_tables(r));
        r.dbg.mark("interpreter tables");
        spec_choose(r);
        if (r.use_spec) RDF_TRY(spec_tables(r));
        r.dbg.mark("specialised tables");
        if (!r.grouped && !r.use_spec) RDF_TRY(eval_tables(r));
        const rdf_status st = r.grouped ? run_group(r) : ps.sink == RDF_SINK_AGG ? run_agg(r) : run_store(r);
        if (st != kRetryInterpreted) return st;
    }
}

// one-node-per-op helper for the single-kernel entry points
rdf_expr_node node_col(int c) { rdf_expr_node n; memset(&n, 0, sizeof n); n.kind = RDF_NODE_COLUMN; n.column = c; n.lhs = n.rhs = -1; return n; }
rdf_expr_node node_op(int op, int l, int r, int dtype = 0) { rdf_expr_node n; memset(&n, 0, sizeof n); n.kind = RDF_NODE_OP; n.op = op; n.lhs = l; n.rhs = r; n.dtype = dtype; return n; }

rdf_status pipeline_stream(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_agg_result* aggs, const char* msg);   // rdf_capi_stream.inc
int64_t host_input_bytes(const rdf_array* cols, int32_t ncols, int64_t nchunks);
int64_t stream_slab_bytes();
rdf_status pipeline_stream_store(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_out* outs, const char* msg);
rdf_status group_pipeline_stream(const ProgramSpec& ps, const rdf_array* cols, int32_t ncols, int64_t nchunks, const char* msg);
rdf_status filter_stream(const rdf_expr_node* nodes, int32_t nnodes, int32_t root, const rdf_array* cols, int32_t ncols, int64_t nchunks, rdf_out* outs);
rdf_status groupby_stream(const rdf_array* keys, const rdf_array* values, int64_t nchunks, int32_t agg, int64_t max_groups,
                          rdf_out* out_keys, rdf_out* out_values, rdf_out* out_counts, int64_t slack);

// Every entry point that takes chunk lists comes through here.  Host-resident batches beyond one slab are streamed (slab k + 1
// crosses the link while the kernel runs over slab k, and — for sinks that materialise on the host — slab k - 1's results
// leave on a third stream): aggregates, new columns / masks, the fused grouped aggregation.  Anything else is one run_program.
rdf_status run_program_any(const ProgramSpec& ps, const rdf_array* cols, int ncols, int64_t nchunks, rdf_out* outs, rdf_agg_result* aggs, const char* msg) {
    g_ctx.stream_slabs = 0;
    if (cols && ncols >= 1 && ncols <= kMaxCols && nchunks >= 1 && g_ctx.opt_stream_slab >= 0) {
        bool host = true;
        for (int64_t i = 0; i < (int64_t)ncols * nchunks && host; ++i) host = cols[i].mem == RDF_MEM_HOST && cols[i].length >= 0 && cols[i].offset >= 0 && (cols[i].length == 0 || cols[i].values);
        if (host && host_input_bytes(cols, ncols, nchunks) > stream_slab_bytes()) {
            if (ps.sink == RDF_SINK_AGG && aggs) return pipeline_stream(ps, cols, ncols, nchunks, aggs, msg);
            if (ps.sink == RDF_SINK_GROUP && ps.gout && ps.ngroups >= 1 && ps.nvalues >= 1 && (int64_t)(ps.ngroups + 1) * ps.nvalues <= RDF_MAX_GROUP_SLOTS)
                return group_pipeline_stream(ps, cols, ncols, nchunks, msg);
            if (ps.sink == RDF_SINK_STORE && outs && ps.nvalues == 1 && ps.filter_root < 0 && !ps.frame_outs) {
                bool ohost = true;
                for (int64_t c = 0; c < nchunks && ohost; ++c) ohost = outs[c].mem == RDF_MEM_HOST;
                if (ohost) return pipeline_stream_store(ps, cols, ncols, nchunks, outs, msg);
            }
        }
    }
    return run_program(ps, cols, ncols, nchunks, outs, aggs, msg);
}

rdf_status agg_column(const rdf_array* a, int64_t nchunks, bool as_f64, rdf_agg_result* r) {
    rdf_expr_node nodes[2] = {node_col(0), node_op(RDF_OP_CAST, 0, -1, RDF_F64)};
    ProgramSpec ps;
    memset(&ps, 0, sizeof ps);
    ps.nodes = nodes; ps.nnodes = 2; ps.filter_root = -1; ps.nvalues = 1; ps.value_roots[0] = as_f64 ? 1 : 0; ps.sink = RDF_SINK_AGG;
    return run_program_any(ps, a, 1, nchunks, nullptr, r, "chunk length mismatch");
}

void store_native(void* out, int dt, const rdf_agg_result& r, int which /*0 sum 1 min 2 max*/) {
    if (is_float(dt)) {
        const double v = which == 0 ? r.sum_f64 : which == 1 ? r.min_f64 : r.max_f64;
        if (dt == RDF_F64) *(double*)out = v; else *(float*)out = (float)v;
        return;
    }
    const int64_t v = which == 0 ? r.sum_i64 : which == 1 ? r.min_i64 : r.max_i64;
    switch (dtype_size(dt)) {
        case 1: *(uint8_t*)out = (uint8_t)v; break;
        case 2: *(uint16_t*)out = (uint16_t)v; break;
        case 4: *(uint32_t*)out = (uint32_t)v; break;
        default: *(uint64_t*)out = (uint64_t)v; break;
    }
}

rdf_status agg_entry(const rdf_array* a, int64_t nchunks, void* out_scalar, int32_t* out_is_some, int which, const char* name) {
    if (!out_scalar || !out_is_some) return fail(RDF_INVALID_ARGUMENT, "%s: null output pointer", name);
    // a column always has at least one chunk (ChunkedArray::from_arrays asserts, src/table.rs:25)
    if (nchunks < 1 || !a) return fail(RDF_INVALID_ARGUMENT, "%s: a column has at least one chunk", name);
    if (!is_numeric(a[0].dtype)) return fail(RDF_INVALID_ARGUMENT, "%s: numeric type required", name);
    rdf_agg_result r;
    RDF_TRY(agg_column(a, nchunks, false, &r));
    if (which == 0) { store_native(out_scalar, a[0].dtype, r, 0); *out_is_some = 1; }
    else { *out_is_some = r.is_some; if (r.is_some) store_native(out_scalar, a[0].dtype, r, which); }
    return RDF_OK;
}

}  // namespace
