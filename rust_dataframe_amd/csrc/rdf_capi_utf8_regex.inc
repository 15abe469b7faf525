// rdf_capi_utf8_regex.inc — host side of rdf_utf8_regexp_info / _match / _count / _extract / _replace / _split (kernels:
// rdf_utf8_regex.hip; the compiler and what is decided about one row: rdf_utf8_regex.h); textually included by rdf_capi.cpp
// after rdf_capi_utf8_rewrite.inc.  A pattern compiles ONCE per call on the host into the image of two DFAs; rlike and
// count then run through utf8_pred_run (the predicates' checks, staging and outputs), the three text operations through
// utf8_rewrite_run (the rewrites' checks, scans, sizing rule and outputs), each with the image in place of a literal.
// Every refusal that concerns the pattern, the group or the replacement comes before any of that, so before any device work.

namespace {

// pattern pointer and length, then the compile: the refusal names the construct and its byte in the pattern
rdf_status utf8_regex_compile_checked(const char* fn, const uint8_t* pattern, int64_t pattern_bytes, Utf8RegexCompiled* out) {
    if (pattern_bytes < 0) return fail(RDF_INVALID_ARGUMENT, "%s: negative pattern length %lld", fn, (long long)pattern_bytes);
    if (pattern_bytes > RDF_UTF8_PATTERN_MAX) return fail(RDF_INVALID_ARGUMENT, "%s: a pattern of %lld bytes, at most %d", fn, (long long)pattern_bytes, RDF_UTF8_PATTERN_MAX);
    if (!pattern && pattern_bytes > 0) return fail(RDF_INVALID_ARGUMENT, "%s: null pattern", fn);
    *out = utf8_regex_compile(pattern, pattern_bytes);
    if (out->status == U8X_SYNTAX) return fail(RDF_INVALID_ARGUMENT, "%s: the pattern holds %s at byte %lld", fn, out->what.c_str(), (long long)out->pos);
    if (out->status != U8X_OK) return fail(RDF_INVALID_ARGUMENT, "%s: the pattern needs %s", fn, out->what.c_str());
    return RDF_OK;
}

}  // namespace

extern "C" {

rdf_status rdf_utf8_regexp_info(const uint8_t* pattern, int64_t pattern_bytes, rdf_regexp_info* out) {
    const char* fn = "utf8_regexp_info";
    if (!out) return fail(RDF_INVALID_ARGUMENT, "%s: null out", fn);
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    out->program_len = rx.h.program_len;
    out->forward_states = rx.h.fwd_states;
    out->reverse_states = rx.h.rev_states;
    out->classes = rx.h.classes;
    out->table_bytes = rx.h.table_bytes;
    out->can_match_empty = rx.h.can_match_empty;
    out->anchored_start = rx.h.anchored_start;
    return RDF_OK;
}

rdf_status rdf_utf8_regexp_match(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, rdf_out* mask) {
    const char* fn = "utf8_regexp_match";
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    Utf8PredCall q = {fn, UTF8_FAM_SCAN, 0, 0, 0, chunks, nullptr, nchunks, nullptr, mask, rx.image.data(), (int64_t)rx.image.size()};
    return utf8_pred_run(q);
}

rdf_status rdf_utf8_regexp_count(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, rdf_out* out) {
    const char* fn = "utf8_regexp_count";
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    Utf8PredCall q = {fn, UTF8_FAM_SCAN, 1, 0, 0, chunks, nullptr, nchunks, nullptr, out, rx.image.data(), (int64_t)rx.image.size()};
    return utf8_pred_run(q);
}

rdf_status rdf_utf8_regexp_extract(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, int32_t group,
                                   rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_regexp_extract";
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    if (group != 0) return fail(RDF_INVALID_ARGUMENT, "%s: group %d: capture groups are not built", fn, group);
    const Utf8RewriteCall q = {fn, U8R_REPLACE, chunks, nchunks, nullptr, 0, nullptr, 0, 0, nullptr, out_offsets, out_data, rx.image.data(), (int64_t)rx.image.size(), U8X_EXTRACT};
    return utf8_rewrite_run(q);
}

rdf_status rdf_utf8_regexp_replace(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, const uint8_t* replacement,
                                   int64_t replacement_bytes, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_regexp_replace";
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    RDF_TRY(utf8_build_check_literal(fn, "the replacement", replacement, replacement_bytes));
    uint8_t rep[RDF_UTF8_PATTERN_MAX + 1];
    int64_t rep_bytes = 0;
    bool dollar = false;
    const int64_t bad = utf8_regex_replacement(replacement, replacement_bytes, rep, &rep_bytes, &dollar);
    if (bad >= 0)
        return fail(RDF_INVALID_ARGUMENT, dollar ? "%s: the replacement holds an unescaped $ at byte %lld: capture groups are not built" : "%s: the replacement ends in a lone backslash at byte %lld",
                    fn, (long long)bad);
    const Utf8RewriteCall q = {fn, U8R_REPLACE, chunks, nchunks, nullptr, 0, rep, rep_bytes, 0, nullptr, out_offsets, out_data, rx.image.data(), (int64_t)rx.image.size(), U8X_REPLACE};
    return utf8_rewrite_run(q);
}

rdf_status rdf_utf8_regexp_split(const rdf_utf8_array* chunks, int64_t nchunks, const uint8_t* pattern, int64_t pattern_bytes, int64_t limit,
                                 rdf_out* out_list_offsets, rdf_out* out_offsets, rdf_out* out_data) {
    const char* fn = "utf8_regexp_split";
    Utf8RegexCompiled rx;
    RDF_TRY(utf8_regex_compile_checked(fn, pattern, pattern_bytes, &rx));
    const Utf8RewriteCall q = {fn, U8R_SPLIT, chunks, nchunks, nullptr, 0, nullptr, 0, limit, out_list_offsets, out_offsets, out_data, rx.image.data(), (int64_t)rx.image.size(), U8X_SPLIT};
    return utf8_rewrite_run(q);
}

}  // extern "C"
