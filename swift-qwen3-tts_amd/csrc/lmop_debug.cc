// lmop_debug.cc -- q3tts_debug_lmop (q3tts.h): one launch of a row kernel of the LM side of the frame step (kernels/sampler.hip,
// kernels/lm_misc.hip, the jobs of kernels/row_jobs.h) on host buffers, through its own launcher. The host checks need neither an
// engine nor a GPU.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "common.h"
#include "engine.h"
#include "kernels.h"

namespace q3 {

namespace {

constexpr int kIn = 14, kIo = 18;
constexpr int64_t kPool = -1;             // a slot of any whole number of bf16
constexpr int64_t kMaxElems = int64_t(1) << 27;
constexpr int kMaxP = 1 << 24;

// the records of q3tts.h are the kernels' own
static_assert(sizeof(q3tts_lm_sampling_params) == sizeof(SamplingParams) && offsetof(q3tts_lm_sampling_params, seed) == offsetof(SamplingParams, seed) &&
                  offsetof(q3tts_lm_sampling_params, mask_eos) == offsetof(SamplingParams, mask_eos) &&
                  offsetof(q3tts_lm_sampling_params, rep_penalty) == offsetof(SamplingParams, rep_penalty),
              "q3tts_lm_sampling_params is SamplingParams");
static_assert(sizeof(q3tts_lm_admit_desc) == sizeof(AdmitDesc) && offsetof(q3tts_lm_admit_desc, sp) == offsetof(AdmitDesc, sp) &&
                  offsetof(q3tts_lm_admit_desc, text_open) == offsetof(AdmitDesc, text_open),
              "q3tts_lm_admit_desc is AdmitDesc");
static_assert(sizeof(q3tts_lm_text_desc) == sizeof(TextAppendDesc) && offsetof(q3tts_lm_text_desc, max_frames) == offsetof(TextAppendDesc, max_frames),
              "q3tts_lm_text_desc is TextAppendDesc");

// What an op's shape states: bytes per slot (0: the slot must be NULL), and which slots may be left out.
struct Plan {
    int64_t in[kIn] = {}, io[kIo] = {};
    bool in_opt[kIn] = {}, io_opt[kIo] = {};
};

#define LM_CHECK(cond, msg) Q3_CHECK(cond, 3, "debug_lmop: " msg)

void check_slots(const q3tts_lmop_debug& d, const Plan& pl) {
    auto one = [](const void* p, int64_t bytes, int64_t need, bool opt) {
        if (need == 0) {
            LM_CHECK(p == nullptr && bytes == 0, "a slot the op does not name must be NULL");
            return;
        }
        if (!p) {
            LM_CHECK(opt && bytes == 0, "null argument");
            return;
        }
        if (need == kPool) LM_CHECK(bytes >= 2 && bytes % 2 == 0 && bytes / 2 <= kMaxElems, "a pool holds whole bf16");
        else LM_CHECK(bytes == need, "a buffer's size disagrees with the strides and counts given");
    };
    for (int i = 0; i < kIn; ++i) one(d.in[i], d.in_bytes[i], pl.in[i], pl.in_opt[i]);
    for (int i = 0; i < kIo; ++i) one(d.io[i], d.io_bytes[i], pl.io[i], pl.io_opt[i]);
}

const int32_t* i32(const void* p) { return static_cast<const int32_t*>(p); }
const int64_t* i64(const void* p) { return static_cast<const int64_t*>(p); }

// a * b * c * e elements of `size` bytes; every factor is at most 2^24 and the running product at most 2^27: no overflow
int64_t bytes_of(int64_t size, int64_t a, int64_t b = 1, int64_t c = 1, int64_t e = 1) {
    int64_t n = 1;
    for (const int64_t v : {a, b, c, e}) {
        LM_CHECK(v >= 1 && v <= kMaxElems, "tensor beyond 2^27 elements");
        n *= v;
        LM_CHECK(n <= kMaxElems, "tensor beyond 2^27 elements");
    }
    return n * size;
}
int64_t strided(int64_t rows, int64_t ld, int64_t dim) { return bytes_of(2, (rows - 1) * ld + dim); }  // bf16 rows, the last one `dim` wide

void batch(int B) { LM_CHECK(B >= 1 && B <= 64, "batch / slots / k out of range (1..64)"); }
void tiled(int rows, int H, int MB) {
    LM_CHECK(H >= 128 && H % 128 == 0 && H <= 8192, "a tiled buffer's width must be a multiple of 128, at most 8192");
    LM_CHECK(MB >= 1 && MB <= 64 && rows >= 1 && rows <= MB * 16, "rows outside a tiled buffer's row blocks");
}
void in_range(const void* v, int64_t n, int64_t lo, int64_t hi, const char* msg) {  // lo <= v[i] < hi
    for (int64_t i = 0; i < n; ++i) Q3_CHECK(i32(v)[i] >= lo && i32(v)[i] < hi, 3, msg);
}

// codec_emb [Vt][H], cp_emb[0 .. groups - 2] [Vcp][H] and (with_pad) a last row [H], by offset into a pool of bf16
void check_tables(const void* offs, int64_t pool_bytes, int groups, int H, int Vt, int Vcp, bool with_pad) {
    const int64_t pool = pool_bytes / 2;
    for (int g = 0; g < groups + (with_pad ? 1 : 0); ++g) {
        const int64_t off = i64(offs)[g], rows = g == 0 ? Vt : (g < groups ? Vcp : 1);
        LM_CHECK(off >= 0 && off % 8 == 0 && off <= pool && off + rows * H <= pool, "a table is not 16-byte aligned or ends outside the pool");
    }
}
// cur_codes [n][16]: group g's code inside group g's table
void check_cur_codes(const void* cc, int n, int groups, int Vt, int Vcp) {
    for (int b = 0; b < n; ++b)
        for (int g = 0; g < groups; ++g) {
            const int c = i32(cc)[b * 16 + g];
            LM_CHECK(c >= 0 && c < (g == 0 ? Vt : Vcp), "cur_codes: a code outside its table");
        }
}

// ops 0 and 1: the sampler's slots
void plan_sampler(const q3tts_lmop_debug& d, Plan& pl) {
    const int32_t* p = d.p;
    const int B = p[0], V = p[1], ldl = p[2], cb = p[7], Fmax = p[9], ff = p[10], emb_rows = p[11], emb_ld = p[12], H = p[13];
    const int next_MB = p[14], next_row0 = p[15], nss = p[16], next_ss_ld = p[17], dump_ld = p[18], dump_off = p[19];
    batch(B);
    LM_CHECK(V >= 1 && V <= 4096 && ldl >= V, "sampler: 1 <= V <= 4096, ldl >= V");
    LM_CHECK((p[3] == 0 || p[3] == 1) && (p[8] == 0 || p[8] == 1) && cb >= 0 && cb <= 15, "sampler: is_talker / advance are flags, cb in 0..15");
    LM_CHECK(p[6] >= -1 && p[6] < V, "sampler: eos_id in -1 .. V - 1");
    LM_CHECK(Fmax >= 0 && ff >= 0 && dump_ld >= 0 && nss >= 0, "sampler: a count is negative");
    pl.in[0] = bytes_of(2, B, ldl);
    pl.in[1] = B * int64_t(sizeof(SamplingParams));
    pl.in[2] = B * 4; pl.in_opt[2] = true;
    pl.in[3] = B; pl.in_opt[3] = true;
    pl.in[7] = B * 4; pl.in_opt[7] = true;
    pl.io[0] = B * 4; pl.io[1] = B; pl.io[2] = B; pl.io[3] = B * 4; pl.io[4] = B * 64;
    if (Fmax > 0) pl.io[5] = bytes_of(4, B, Fmax, 16);
    pl.io[6] = bytes_of(1, B, V); pl.io_opt[6] = true;
    if (ff > 0) {
        pl.in[4] = pl.io[7] = bytes_of(4, B, ff, 16);
        pl.in_opt[4] = pl.io_opt[7] = true;
        if (dump_ld > 0) {
            LM_CHECK(dump_off >= 0 && dump_off + V <= dump_ld, "sampler: dump_off + V must not exceed dump_ld");
            pl.io[8] = bytes_of(2, B, ff, dump_ld); pl.io_opt[8] = true;
        }
    }
    if (H > 0) {  // the gather of the next input
        LM_CHECK(emb_ld >= H && emb_ld % 8 == 0 && emb_rows >= V, "sampler: emb_ld >= H in whole 16-byte pieces, emb_rows >= V (any token may be drawn)");
        LM_CHECK(next_row0 >= 0, "sampler: next_row0 is negative");
        tiled(next_row0 + B, H, next_MB);
        pl.in[5] = bytes_of(2, emb_rows, emb_ld);
        pl.io[9] = bytes_of(2, next_MB * 16, H);
        if (d.in[6]) {
            LM_CHECK(nss >= 1 && next_ss_ld >= next_row0 + B, "sampler: emb_ss needs nss >= 1 and next_ss_ld >= next_row0 + B");
            pl.in[6] = bytes_of(4, emb_rows, nss);
            pl.io[10] = bytes_of(4, nss, next_ss_ld);
        } else {
            pl.io[10] = B * 4; pl.io_opt[10] = true;
        }
    }
}
void check_sampler_values(const q3tts_lmop_debug& d) {
    const int32_t* p = d.p;
    in_range(d.io[0], p[0], 0, kMaxP + 1, "debug_lmop: n_frames outside 0 .. 2^24");
    if (d.in[4]) in_range(d.in[4], int64_t(p[0]) * p[10] * 16, 0, p[1], "debug_lmop: sampler: a forced code outside 0 .. V - 1");
}

// ops 1 and 2: the end-of-frame job's slots
void plan_frame_end(const q3tts_lmop_debug& d, Plan& pl, bool own_cp_len) {
    const int32_t* p = d.p;
    const int B = p[0], H = p[20], groups = p[21], Tmax = p[22], hMB = p[23], Vt = p[24], Vcp = p[25];
    batch(B);
    tiled(B, H, hMB);
    LM_CHECK(groups >= 1 && groups <= 16 && Tmax >= 1 && Vt >= 1 && Vcp >= 1, "frame_end: groups in 1..16, Tmax, Vt, Vcp >= 1");
    pl.in[2] = B * 4; pl.in_opt[2] = false;
    pl.in[8] = kPool;
    pl.in[9] = (groups + 1) * 8;
    pl.in[10] = bytes_of(2, B, Tmax, H);
    pl.in[11] = B * 4;
    pl.in[12] = B; pl.in_opt[12] = true;
    pl.io[0] = B * 4; pl.io[1] = B; pl.io[2] = B; pl.io[4] = B * 64;
    pl.io[11] = B * 4;
    pl.io[12] = bytes_of(2, hMB * 16, H);
    pl.io[13] = B * 4;
    if (own_cp_len) pl.io[14] = B * 4;
    pl.io[15] = B; pl.io_opt[15] = true;
}
void check_frame_end_values(const q3tts_lmop_debug& d) {
    const int32_t* p = d.p;
    const int B = p[0], groups = p[21];
    LM_CHECK((d.in[12] != nullptr) == (d.io[15] != nullptr), "frame_end: text_open and starved come together");
    check_tables(d.in[9], d.in_bytes[8], groups, p[20], p[24], p[25], true);
    check_cur_codes(d.io[4], B, groups, p[24], p[25]);
    in_range(d.in[11], B, 0, p[22] + 1, "debug_lmop: frame_end: n_trailing outside 0 .. Tmax");
    in_range(d.io[11], B, 0, kMaxP + 1, "debug_lmop: frame_end: trailing_idx outside 0 .. 2^24");
    in_range(d.io[0], B, 0, kMaxP + 1, "debug_lmop: n_frames outside 0 .. 2^24");
}

}  // namespace

void Engine::debug_lmop_check(const q3tts_lmop_debug& d) {
    LM_CHECK(d.op >= 0 && d.op <= 18, "unknown op");
    const int32_t* p = d.p;
    for (int i = 0; i < 32; ++i)
        LM_CHECK((d.op == 18 && (i == 1 || i == 2)) || (p[i] >= -kMaxP && p[i] <= kMaxP), "parameter out of range");
    Plan pl;
    switch (d.op) {
        case 0: {  // sampler
            plan_sampler(d, pl);
            check_slots(d, pl);
            check_sampler_values(d);
            break;
        }
        case 1: {  // sampler with the end-of-frame job riding along, or the two launches it replaces
            LM_CHECK(p[3] == 0 && p[1] <= 2048, "sampler + frame end: a code-predictor draw (is_talker 0, V <= 2048)");
            LM_CHECK((p[26] == 0 || p[26] == 1) && (p[27] == 0 || p[27] == 1), "sampler + frame end: split / cp_len_is_kv_len are flags");
            plan_sampler(d, pl);
            plan_frame_end(d, pl, p[27] == 0);
            // the draw is the frame's last: its code is group groups - 1's, whatever is drawn or forced
            LM_CHECK(p[21] >= 2 && p[7] == p[21] - 1 && p[1] <= p[25], "sampler + frame end: groups >= 2, cb = groups - 1, V within that group's table");
            check_slots(d, pl);
            check_sampler_values(d);
            check_frame_end_values(d);
            break;
        }
        case 2: {  // frame_end
            plan_frame_end(d, pl, true);
            check_slots(d, pl);
            check_frame_end_values(d);
            break;
        }
        case 3: {  // gather_rows
            const int n = p[0], rows = p[1], ld = p[2], dim = p[3], ldo = p[4], out_MB = p[5], map_n = p[6];
            LM_CHECK(n >= 1 && n <= 4096 && rows >= 1 && dim >= 8 && dim % 8 == 0 && ld >= dim && ld % 8 == 0 && map_n >= 0,
                     "gather_rows: dim and ld in whole 16-byte pieces, ld >= dim");
            pl.in[0] = bytes_of(2, rows, ld); pl.in[1] = n * 4;
            if (map_n > 0) pl.in[2] = bytes_of(4, map_n);
            if (out_MB > 0) {
                tiled(n, dim, out_MB);
                pl.io[0] = bytes_of(2, out_MB * 16, dim);
            } else {
                LM_CHECK(out_MB == 0 && ldo >= dim && ldo % 8 == 0, "gather_rows: ldo >= dim in whole 16-byte pieces");
                pl.io[0] = bytes_of(2, n, ldo);
            }
            check_slots(d, pl);
            in_range(d.in[1], n, 0, map_n > 0 ? map_n : rows, "debug_lmop: gather_rows: an id outside the table / token map");
            if (map_n > 0) in_range(d.in[2], map_n, 0, rows, "debug_lmop: gather_rows: a token_map value outside the table");
            break;
        }
        case 4: case 5: {  // tile_rows, untile_rows
            const int rows = p[0], dim = p[1], ld = d.op == 4 ? p[2] : p[3], MB = d.op == 4 ? p[3] : p[2];
            tiled(rows, dim, MB);
            LM_CHECK(ld >= dim && ld % 8 == 0, "tile / untile: ld >= dim in whole 16-byte pieces");
            (d.op == 4 ? pl.in[0] : pl.io[0]) = bytes_of(2, rows, ld);
            (d.op == 4 ? pl.io[0] : pl.in[0]) = bytes_of(2, MB * 16, dim);
            check_slots(d, pl);
            break;
        }
        case 6: {  // add_rows
            const int rows = p[0], dim = p[1], lda = p[2], ldb = p[3], ldo = p[4];
            LM_CHECK(rows >= 1 && dim >= 1 && lda >= dim && ldo >= dim && (ldb == 0 || ldb >= dim), "add_rows: ld >= dim (ldb: or 0)");
            pl.in[0] = bytes_of(2, rows, lda);
            pl.in[1] = ldb == 0 ? bytes_of(2, dim) : bytes_of(2, rows, ldb);
            pl.io[0] = bytes_of(2, rows, ldo);
            check_slots(d, pl);
            break;
        }
        case 7: {  // compose_rows
            const int n = p[0], dim = p[1], proj_rows = p[2], ldp = p[3], table_rows = p[4], ldt = p[5], extra_rows = p[6], lde = p[7];
            const int dst_rows = p[8], ldd = p[9];
            LM_CHECK(n >= 1 && n <= 4096 && dim >= 1 && ldp >= dim && ldt >= dim && ldd >= dim && extra_rows >= 0, "compose_rows: ld >= dim");
            pl.in[0] = bytes_of(2, proj_rows, ldp); pl.in[1] = bytes_of(2, table_rows, ldt);
            if (extra_rows > 0) {
                LM_CHECK(lde >= dim, "compose_rows: lde >= dim");
                pl.in[2] = bytes_of(2, extra_rows, lde);
            }
            pl.in[3] = pl.in[4] = pl.in[5] = n * 4;
            pl.io[0] = bytes_of(2, dst_rows, ldd);
            check_slots(d, pl);
            in_range(d.in[3], n, 0, proj_rows, "debug_lmop: compose_rows: a[i] outside proj");
            in_range(d.in[4], n, -1 - int64_t(extra_rows), table_rows, "debug_lmop: compose_rows: b[i] outside table / extra");
            in_range(d.in[5], n, 0, dst_rows, "debug_lmop: compose_rows: dst_row[i] outside dst");
            std::vector<int32_t> rows(i32(d.in[5]), i32(d.in[5]) + n);
            std::sort(rows.begin(), rows.end());
            LM_CHECK(std::adjacent_find(rows.begin(), rows.end()) == rows.end(), "compose_rows: two rows with one destination");
            break;
        }
        case 8: {  // ref_embed_rows
            const int T = p[0], groups = p[1], H = p[2], ldo = p[3], Vt = p[4], Vcp = p[5];
            LM_CHECK(T >= 1 && T <= 4096 && groups >= 1 && groups <= 16 && H >= 1 && ldo >= H && Vt >= 1 && Vcp >= 1, "ref_embed_rows: sizes out of range");
            pl.in[0] = bytes_of(4, groups, T); pl.in[1] = kPool; pl.in[2] = groups * 8;
            pl.io[0] = bytes_of(2, T, ldo);
            check_slots(d, pl);
            check_tables(d.in[2], d.in_bytes[1], groups, H, Vt, Vcp, false);
            in_range(d.in[0], T, 0, Vt, "debug_lmop: ref_embed_rows: a code outside codec_emb");
            in_range(i32(d.in[0]) + T, int64_t(groups - 1) * T, 0, Vcp, "debug_lmop: ref_embed_rows: a code outside its cp_emb table");
            break;
        }
        case 9: {  // f32_to_bf16
            pl.in[0] = bytes_of(4, p[0]); pl.io[0] = bytes_of(2, p[0]);
            check_slots(d, pl);
            break;
        }
        case 10: {  // ss_to_table
            const int rows = p[0], nss = p[1], ss_ld = p[2];
            LM_CHECK(rows >= 1 && nss >= 1 && ss_ld >= rows, "ss_to_table: ss_ld >= rows");
            pl.in[0] = bytes_of(4, nss, ss_ld); pl.io[0] = bytes_of(4, rows, nss);
            check_slots(d, pl);
            break;
        }
        case 11: {  // copy_rows
            const int rows = p[0], dim = p[1], lds = p[2], ldd = p[3];
            LM_CHECK(rows >= 1 && rows <= 4096 && dim >= 8 && dim % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0, "copy_rows: dim and strides in whole 16-byte pieces");
            LM_CHECK((lds == 0 || lds >= dim) && (ldd >= dim || (ldd == 0 && rows == 1)), "copy_rows: a stride is 0 (lds; ldd with one row) or at least dim");
            pl.in[0] = strided(rows, lds, dim); pl.io[0] = strided(rows, ldd, dim);
            check_slots(d, pl);
            break;
        }
        case 12: case 13: {  // prefill_load, prefill_chunk_load
            const int B = p[0], Pmax = p[1], step = p[2], H = p[3], hMB = p[4], C = d.op == 13 ? p[5] : 1;
            batch(B);
            LM_CHECK(Pmax >= 1 && C >= 1 && C <= 64, "prefill load: Pmax >= 1, 1 <= C <= 64");
            tiled(C * B, H, hMB);
            pl.in[0] = bytes_of(2, B, Pmax, H); pl.in[1] = B * 4;
            pl.io[0] = bytes_of(2, hMB * 16, H); pl.io[1] = C * B * 4;
            if (d.op == 12) pl.io[2] = B;
            check_slots(d, pl);
            in_range(d.in[1], B, 0, Pmax + 1, "debug_lmop: prefill load: n_prompt outside 0 .. Pmax");
            for (int b = 0; b < B; ++b) {  // the last position the launch loads for row b
                const int64_t np = i32(d.in[1])[b], last = d.op == 12 ? int64_t(step) - (Pmax - np) : int64_t(step) + np + C - 1;
                LM_CHECK(last < Pmax, "prefill load: a prompt position at or beyond Pmax");
            }
            break;
        }
        case 14: case 15: {  // advance_len, advance_len_chunk
            const int B = p[0];
            batch(B);
            if (d.op == 14) { pl.in[0] = B; pl.in_opt[0] = true; }
            else {
                LM_CHECK(p[2] >= 1, "advance_len_chunk: C >= 1");
                pl.in[0] = B * 4;
            }
            pl.io[0] = B * 4;
            check_slots(d, pl);
            break;
        }
        case 16: {  // admit_rows
            const int k = p[0], slots = p[1], H = p[2], V = p[3], Fmax = p[4], srcMB = p[5], hMB = p[6];
            batch(k); batch(slots);
            tiled(k, H, srcMB); tiled(slots, H, hMB);
            LM_CHECK(V >= 1 && V <= 4096 && Fmax >= 1, "admit_rows: 1 <= V <= 4096, Fmax >= 1");
            pl.in[0] = k * int64_t(sizeof(AdmitDesc)); pl.in[1] = bytes_of(2, srcMB * 16, H); pl.in[2] = pl.in[3] = pl.in[4] = k * 4;
            pl.io[0] = bytes_of(2, hMB * 16, H);
            for (int i = 1; i <= 8; ++i) pl.io[i] = slots * 4;
            pl.io[9] = slots * 64; pl.io[10] = bytes_of(4, slots, Fmax, 16); pl.io[11] = slots * 4;
            pl.io[12] = slots * int64_t(sizeof(SamplingParams));
            pl.io[13] = pl.io[14] = slots; pl.io[15] = bytes_of(1, slots, V);
            pl.io[16] = pl.io[17] = slots; pl.io_opt[16] = pl.io_opt[17] = true;
            check_slots(d, pl);
            uint64_t taken = 0;
            for (int j = 0; j < k; ++j) {
                const int s = static_cast<const AdmitDesc*>(d.in[0])[j].slot;
                LM_CHECK(s >= -1 && s < slots, "admit_rows: a slot outside -1 .. slots - 1");
                if (s < 0) continue;
                LM_CHECK(!((taken >> s) & 1), "admit_rows: two rows for one slot");
                taken |= uint64_t(1) << s;
            }
            break;
        }
        case 17: {  // text_append_rows
            const int k = p[0], slots = p[1], H = p[2], Tmax = p[3], groups = p[4], hMB = p[5], Vt = p[6], Vcp = p[7], src_rows = p[8];
            batch(k); batch(slots);
            tiled(slots, H, hMB);
            LM_CHECK(groups >= 1 && groups <= 16 && Tmax >= 1 && Vt >= 1 && Vcp >= 1 && src_rows >= 1, "text_append_rows: sizes out of range");
            pl.in[0] = k * int64_t(sizeof(TextAppendDesc)); pl.in[1] = bytes_of(2, src_rows, H); pl.in[2] = H * 2; pl.in[3] = kPool;
            pl.in[4] = (groups + 1) * 8; pl.in[5] = slots * 64;
            pl.io[0] = bytes_of(2, slots, Tmax, H); pl.io[1] = slots * 4; pl.io[2] = slots; pl.io[3] = slots * 4; pl.io[4] = slots * 4;
            pl.io[5] = bytes_of(2, hMB * 16, H); pl.io[6] = slots * 4; pl.io[7] = slots * 4; pl.io[8] = pl.io[9] = pl.io[10] = slots;
            check_slots(d, pl);
            check_tables(d.in[4], d.in_bytes[3], groups, H, Vt, Vcp, true);
            check_cur_codes(d.in[5], slots, groups, Vt, Vcp);
            in_range(d.io[1], slots, 0, Tmax + 1, "debug_lmop: text_append_rows: n_trailing outside 0 .. Tmax");
            in_range(d.io[4], slots, 0, kMaxP + 1, "debug_lmop: text_append_rows: trailing_idx outside 0 .. 2^24");
            uint64_t taken = 0;
            for (int j = 0; j < k; ++j) {
                const TextAppendDesc& t = static_cast<const TextAppendDesc*>(d.in[0])[j];
                LM_CHECK(t.slot >= 0 && t.slot < slots && !((taken >> t.slot) & 1), "text_append_rows: a slot outside 0 .. slots - 1, or listed twice");
                taken |= uint64_t(1) << t.slot;
                LM_CHECK((t.close == 0 || t.close == 1) && t.n_new >= 0 && t.src_row >= 0 && int64_t(t.src_row) + t.n_new <= src_rows && t.n_new + t.close <= Tmax,
                         "text_append_rows: src_row + n_new <= src_rows, n_new + close <= Tmax");
            }
            break;
        }
        default: {  // cancel_rows
            const int slots = p[0], n = p[3];
            batch(slots);
            LM_CHECK(n >= slots && n <= 64, "cancel_rows: slots <= n <= 64");
            pl.io[0] = pl.io[1] = n;
            check_slots(d, pl);
            break;
        }
    }
}

void Engine::debug_lmop(q3tts_lmop_debug& d) {
    debug_lmop_check(d);
    DevBuf<uint8_t> din[kIn], dio[kIo], dtab;
    const uint8_t* in[kIn] = {};
    uint8_t* io[kIo] = {};
    for (int i = 0; i < kIn; ++i)
        if (d.in[i]) {
            in[i] = din[i].grow(size_t(d.in_bytes[i]));
            Q3_HIP(hipMemcpy(din[i], d.in[i], size_t(d.in_bytes[i]), hipMemcpyHostToDevice));
        }
    for (int i = 0; i < kIo; ++i)
        if (d.io[i]) {
            io[i] = dio[i].grow(size_t(d.io_bytes[i]));
            Q3_HIP(hipMemcpy(dio[i], d.io[i], size_t(d.io_bytes[i]), hipMemcpyHostToDevice));
        }
    auto H16 = [&](int i) { return reinterpret_cast<const uint16_t*>(in[i]); };
    auto F = [&](int i) { return reinterpret_cast<const float*>(in[i]); };
    auto I = [&](int i) { return reinterpret_cast<const int32_t*>(in[i]); };
    auto O16 = [&](int i) { return reinterpret_cast<uint16_t*>(io[i]); };
    auto OF = [&](int i) { return reinterpret_cast<float*>(io[i]); };
    auto OI = [&](int i) { return reinterpret_cast<int32_t*>(io[i]); };
    // the device array of 15 cp_emb tables, from offsets into the pool (entries behind groups - 1 are never read: the pool itself)
    auto cp_table = [&](const uint16_t* pool, const int64_t* offs, int groups) {
        std::vector<const uint16_t*> t(15, pool);
        for (int g = 1; g < groups; ++g) t[size_t(g - 1)] = pool + offs[g];
        dtab.grow(15 * sizeof(const uint16_t*));
        Q3_HIP(hipMemcpy(dtab, t.data(), 15 * sizeof(const uint16_t*), hipMemcpyHostToDevice));
        return reinterpret_cast<const uint16_t* const*>(static_cast<uint8_t*>(dtab));
    };
    const int32_t* p = d.p;
    auto sampler_args = [&] {
        SamplerArgs a{};
        a.logits = H16(0); a.ldl = p[2]; a.V = p[1]; a.sp = reinterpret_cast<const SamplingParams*>(in[1]);
        a.is_talker = p[3]; a.suppress_lo = p[4]; a.suppress_hi = p[5]; a.eos_id = p[6];
        a.seen = io[6]; a.cb = p[7]; a.n_frames = OI(0); a.max_frames = I(2); a.finished = io[1]; a.active = io[2];
        a.kv_len = OI(3); a.advance = p[8]; a.advance_gate = in[3]; a.cur_codes = OI(4); a.codes = OI(5); a.Fmax = p[9];
        a.forced = I(4); a.forced_frames = p[10]; a.sampled = OI(7);
        a.emb = H16(5); a.emb_ld = p[12]; a.next_x = O16(9); a.next_MB = p[14]; a.next_row0 = p[15]; a.next_ss = OF(10);
        a.emb_ss = F(6); a.nss = p[16]; a.next_ss_ld = p[17]; a.H = p[13]; a.B = p[0];
        a.logits_dump = O16(8); a.dump_ld = p[18]; a.dump_off = p[19];
        a.row_key = reinterpret_cast<const uint32_t*>(in[7]);
        return a;
    };
    auto frame_end_args = [&] {
        FrameEndArgs a{};
        const int64_t* offs = i64(d.in[9]);
        a.cur_codes = OI(4); a.codec_emb = H16(8) + offs[0]; a.cp_emb = cp_table(H16(8), offs, p[21]);
        a.trailing = H16(10); a.n_trailing = I(11); a.trailing_idx = OI(11); a.Tmax = p[22]; a.tts_pad = H16(8) + offs[p[21]];
        a.h = O16(12); a.hMB = p[23]; a.H = p[20]; a.B = p[0]; a.groups = p[21]; a.ss_out = OF(13);
        a.n_frames = OI(0); a.max_frames = I(2); a.finished = io[1]; a.active = io[2];
        a.cp_len = (d.op == 1 && p[27]) ? OI(3) : OI(14);
        a.text_open = in[12]; a.starved = io[15];
        return a;
    };
    switch (d.op) {
        case 0: launch_sampler(sampler_args(), st_); break;
        case 1: {
            const SamplerArgs sa = sampler_args();
            const FrameEndArgs fe = frame_end_args();
            if (p[26]) {
                launch_sampler(sa, st_);
                launch_frame_end(fe, st_);
            } else {
                launch_sampler_with_frame_end(sa, fe, st_);
            }
            break;
        }
        case 2: launch_frame_end(frame_end_args(), st_); break;
        case 3: launch_gather_rows(H16(0), p[2], I(1), I(2), p[0], p[3], O16(0), p[4], p[5], st_); break;
        case 4: launch_tile_rows(H16(0), p[2], O16(0), p[3], p[0], p[1], st_); break;
        case 5: launch_untile_rows(H16(0), p[2], O16(0), p[3], p[0], p[1], st_); break;
        case 6: launch_add_rows(H16(0), p[2], H16(1), p[3], p[0], p[1], O16(0), p[4], st_); break;
        case 7: launch_compose_rows(H16(0), p[3], H16(1), p[5], H16(2), p[7], I(3), I(4), I(5), O16(0), p[9], p[0], p[1], st_); break;
        case 8: {
            const int64_t* offs = i64(d.in[2]);
            launch_ref_embed_rows(I(0), p[0], p[1], H16(1) + offs[0], cp_table(H16(1), offs, p[1]), p[2], O16(0), p[3], st_);
            break;
        }
        case 9: launch_f32_to_bf16(F(0), O16(0), p[0], st_); break;
        case 10: launch_ss_to_table(F(0), p[2], OF(0), p[1], p[0], st_); break;
        case 11: launch_copy_rows(H16(0), p[2], O16(0), p[3], p[0], p[1], st_); break;
        case 12: case 13: {
            PrefillLoadArgs a{};
            a.prompt = H16(0); a.n_prompt = I(1); a.Pmax = p[1]; a.step = p[2]; a.H = p[3]; a.B = p[0];
            a.h = O16(0); a.hMB = p[4]; a.ss_out = OF(1); a.active = io[2];
            if (d.op == 12) launch_prefill_load(a, st_);
            else launch_prefill_chunk_load(a, p[5], st_);
            break;
        }
        case 14: launch_advance_len(OI(0), in[0], p[0], st_); break;
        case 15: launch_advance_len_chunk(OI(0), I(0), p[1], p[2], p[0], st_); break;
        case 16: {
            AdmitArgs a{};
            a.desc = reinterpret_cast<const AdmitDesc*>(in[0]); a.src_h = H16(1); a.srcMB = p[5]; a.src_ss = F(2); a.src_kv_len = I(3);
            a.src_n_prompt = I(4); a.h = O16(0); a.hMB = p[6]; a.ss = OF(1); a.H = p[2]; a.V = p[3]; a.Fmax = p[4]; a.slots = p[1];
            a.kv_len = OI(2); a.n_prompt = OI(3); a.n_trailing = OI(4); a.max_frames = OI(5); a.n_frames = OI(6); a.cp_len = OI(7);
            a.trailing_idx = OI(8); a.cur_codes = OI(9); a.codes = OI(10); a.row_key = reinterpret_cast<uint32_t*>(io[11]);
            a.sp = reinterpret_cast<SamplingParams*>(io[12]); a.finished = io[13]; a.active = io[14]; a.seen = io[15];
            a.text_open = io[16]; a.starved = io[17];
            launch_admit_rows(a, p[0], st_);
            break;
        }
        case 17: {
            TextAppendArgs a{};
            const int64_t* offs = i64(d.in[4]);
            a.desc = reinterpret_cast<const TextAppendDesc*>(in[0]); a.src = H16(1); a.eos_row = H16(2); a.trailing = O16(0);
            a.n_trailing = OI(1); a.text_open = io[2]; a.max_frames = OI(3); a.slots = p[1];
            FrameEndArgs& fe = a.fe;
            fe.cur_codes = I(5); fe.codec_emb = H16(3) + offs[0]; fe.cp_emb = cp_table(H16(3), offs, p[4]);
            fe.trailing = O16(0); fe.n_trailing = OI(1); fe.trailing_idx = OI(4); fe.Tmax = p[3]; fe.tts_pad = H16(3) + offs[p[4]];
            fe.h = O16(5); fe.hMB = p[5]; fe.H = p[2]; fe.B = p[1]; fe.groups = p[4]; fe.ss_out = OF(6);
            fe.max_frames = OI(3); fe.finished = io[9]; fe.active = io[10]; fe.cp_len = OI(7); fe.text_open = io[2]; fe.starved = io[8];
            launch_text_append_rows(a, static_cast<const TextAppendDesc*>(d.in[0]), p[0], st_);
            break;
        }
        default: {
            const uint64_t mask = (uint64_t(uint32_t(p[2])) << 32) | uint32_t(p[1]);
            launch_cancel_rows(mask, io[0], io[1], p[0], st_);
            break;
        }
    }
    Q3_HIP(hipGetLastError());
    Q3_HIP(hipStreamSynchronize(st_));
    for (int i = 0; i < kIo; ++i)
        if (d.io[i]) Q3_HIP(hipMemcpy(d.io[i], dio[i], size_t(d.io_bytes[i]), hipMemcpyDeviceToHost));
}

}  // namespace q3
