// acgpu_pieces.hip -- how a text is scanned piece by piece into a record reservoir of bounded size: the sizes of the pieces
// (PieceRamp), the reservoir's budget, and the ONE driver (scan_next_piece) behind its six consumers: the cursor
// (acgpu_cursor.hip), the counting entries (acgpu_count.hip), the replace entries (acgpu_replace.hip), the batch summary
// (acgpu_summary.hip), the batch counts per haystack (acgpu_terms.hip) and the spans entries (acgpu_spans.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acgpu_host.h"
#include "acgpu_internal.h"

namespace acgpu {

uint64_t reservoir_budget_bytes() { return (uint64_t)std::max<int64_t>(tunables().cursor_reservoir_bytes.load(std::memory_order_relaxed), 16); }

void PieceRamp::start() {
    piece = (uint64_t)std::max<int64_t>(1, tunables().cursor_first_piece.load(std::memory_order_relaxed));
    seen_records = seen_units = 0;
}

// the next step of the ramp, capped so that the density seen so far fills at most half the reservoir budget
uint64_t PieceRamp::next_size(uint64_t left, uint64_t budget_recs) const {
    uint64_t size = std::min<uint64_t>(piece, left);
    if (seen_records && seen_units) {
        const double per_unit = (double)seen_records / (double)seen_units;
        const double fit = (double)(budget_recs / 2) / per_unit;
        if (fit < (double)size) size = std::max<uint64_t>(1, (uint64_t)fit);
    }
    return size;
}

uint64_t PieceRamp::predicted_room(uint64_t size, uint64_t budget_recs) const {
    if (!seen_units) return 0;
    const double pred = (double)seen_records / (double)seen_units * (double)size;
    return std::min<uint64_t>(budget_recs, (uint64_t)(pred * 1.25) + 1024);
}

bool PieceRamp::on_overflow(uint64_t *size, uint64_t cnt, uint64_t budget_recs, uint64_t *room) const {
    if (cnt <= budget_recs) { // a larger reservoir
        *room = std::min<uint64_t>(budget_recs, cnt + cnt / 8);
    } else if (*size > 1) { // a smaller piece: half the budget by this piece's density
        *size = std::max<uint64_t>(1, (uint64_t)((double)*size * (double)(budget_recs / 2) / (double)cnt));
        *room = budget_recs;
    } else {
        return false;
    }
    return true;
}

void PieceRamp::advance(uint64_t size, uint64_t cnt) {
    seen_records += cnt;
    seen_units += size;
    const uint64_t max_piece = (uint64_t)std::max<int64_t>(1, tunables().cursor_max_piece.load(std::memory_order_relaxed));
    piece = std::min<uint64_t>(max_piece, std::max<uint64_t>(size, 1) * 4);
}

// One scan of the owned units [p.pos, p.pos + size) into p.res as it stands.  ACGPU_OK: *cnt records, p.chain is the exit;
// ACGPU_E_OVERFLOW: *cnt is what did not fit, and a counting host range has moved *done to the position up to which the piece is
// counted all the same (p.chain: the entry into the rest).  *base: the text position of the buffer's unit 0.
int PieceScan::operator()(PieceDriver &p, uint64_t size, uint64_t *cnt, uint64_t *done, uint64_t *base) const {
    const ShardRule rule = shard_rule(a->t, p.record_kind, shard && readable);
    const uint64_t own_hi = p.pos + size;
    *base = 0;
    if (shard) { // the caller's buffer, a moving owned range (readable: a stream's, by the rule of the Readable loops)
        acgpu_shard sh = *shard;
        sh.own_begin = p.pos;
        sh.own_end = own_hi;
        sh.d_result = nullptr;
        const int64_t entry = rule.chain == Chain::None ? shard->chain_entry : piece_entry(rule, p.chain, 0, p.pos);
        sh.chain_entry = entry;
        const int rc = match_shard(a, d, &sh, p.record_kind, p.res->p, p.res->recs, cnt, stream, nullptr, readable);
        if (rc == ACGPU_OK) p.chain = piece_exit(rule, entry, own_hi, &sh, *cnt);
        return rc;
    }
    if (p.whole) { // the text as one shard (the loops that exist only as one sequential kernel)
        acgpu_shard sh;
        const int rc = stage_whole_text(d, hay, n, &sh);
        p.scan_end = n;
        return rc ? rc : match_shard(a, d, &sh, p.record_kind, p.res->p, p.res->recs, cnt, d.call_stream, nullptr);
    }
    const uint64_t lo = p.pos - std::min(rule.left, p.pos), hi = std::min<uint64_t>(n, own_hi + rule.right);
    int64_t chain = p.chain - (int64_t)lo; // (buffer relative: scan_host_range takes each shard's entry from it)
    uint64_t done_rel = p.pos - lo;
    const int rc = scan_host_range(a, d, hay, n, lo, hi, p.pos, own_hi, p.record_kind, p.res->recs, cnt, &chain, p.res->p,
                                   p.through ? &done_rel : nullptr);
    if (rc == ACGPU_OK || (rc == ACGPU_E_OVERFLOW && p.through)) {
        p.chain = chain + (int64_t)lo;
        *done = lo + done_rel;
    }
    *base = lo;
    p.scan_end = std::max(p.scan_end, hi);
    return rc;
}

int scan_next_piece(PieceDriver &p, const PieceScan &scan, uint64_t *n_out, uint64_t *base) {
    const uint64_t rk = (uint64_t)p.record_kind;
    const uint64_t budget_recs = std::max<uint64_t>(reservoir_budget_bytes() / rk, 1);
    uint64_t size = p.whole ? p.end - p.pos : p.ramp.next_size(p.end - p.pos, budget_recs);
    for (;;) {
        // predicted records: room for them (within the budget) before the scan, so that a steady text is not scanned twice;
        // nothing known yet: a record per unit (natural text against a word list has 0.8), of a whole text one per 16 units
        uint64_t room = p.ramp.predicted_room(size, budget_recs);
        if (!room) room = std::min<uint64_t>(budget_recs, std::max<uint64_t>(p.whole ? size / 16 : size, 4096));
        int rc = p.res->ensure(room, rk);
        if (rc) return rc;
        const uint64_t before = p.through ? *p.through : 0;
        uint64_t cnt = 0, done = p.pos;
        rc = scan(p, size, &cnt, &done, base);
        // The ramp's density is what the reservoir has to hold per unit of text: the units of a direct piece count, its records --
        // there are none to hold -- do not, so a text that has gone over to the direct form soon takes the largest pieces.
        const uint64_t held = p.through ? *p.through - before : (rc == ACGPU_OK ? cnt : 0);
        p.pieces++;
        p.units_scanned += size;
        if (rc == ACGPU_E_OVERFLOW) {
            p.rescans++;
            if (done > p.pos) p.ramp.advance(done - p.pos, held); // (the shards in front of the one that did not fit)
            size -= done - p.pos;
            p.pos = done;
            uint64_t want = cnt; // (the one sequential scan: the exact count, past the budget if device memory allows)
            if (!p.whole && !p.ramp.on_overflow(&size, cnt, budget_recs, &want)) return ACGPU_E_NOMEM; // one unit's records do not fit the budget
            if ((rc = p.res->ensure(want, rk))) return rc;
            continue;
        }
        if (rc) return rc;
        p.ramp.advance(size, held);
        p.pos += size;
        *n_out = cnt;
        return ACGPU_OK;
    }
}

} // namespace acgpu
