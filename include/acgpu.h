/*
 * acgpu.h -- C ABI of the MI355X-native multi-pattern matcher (libacgpu.so).
 *
 * This is the drop-in boundary for the hot path of RokLenarcic/AhoCorasick:
 * the reference has no FFI seam of its own -- its seam is the Java interface
 * pair StringSet / StringMap (S/StringSet.java:3-5, S/StringMap.java:5-9) and
 * the listeners (S/SetMatchListener.java:6, S/MapMatchListener.java:6).  A Java
 * facade implementing those interfaces binds exactly the entry points below
 * through JNI (INTEGRATION.md shows the stub); tests and bench.py bind them
 * through ctypes.  S/ = src/main/java/com/roklenarcic/util/strings/.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++ or torch types cross this boundary;
 *  - every function returns ACGPU_OK (0) or a negative ACGPU_E_* code; nothing
 *    throws across the ABI;
 *  - keywords and haystacks are UTF-16 code units exactly as a Java String holds
 *    them; match positions are code-unit indices, `end` exclusive
 *    (R/README.md:69);
 *  - an automaton is immutable after acgpu_build and may be shared by threads;
 *    concurrent matches on one automaton are safe (they serialise on its
 *    per-device scratch pool);
 *  - there is NO CPU matching backend: every acgpu_match_* call needs a HIP
 *    device and fails with ACGPU_E_NODEVICE / ACGPU_E_HIP without one;
 *  - device memory: the tables of an automaton (built once per device; the
 *    reference's 235 886-word README dictionary: 0.5 GB) and a grow-only scratch
 *    pool per automaton and device -- up to 16 bytes per record of the largest
 *    call, and for the matchers that keep a value per haystack unit
 *    (LongestMatch: 1-4 bytes; AhoCorasick on texts with dense matches,
 *    csrc/acgpu_states.hip: 4 bytes) that much per unit of the largest shard.
 *    A pool that cannot grow makes the call take a form that needs less, or
 *    fail with ACGPU_E_NOMEM; acgpu_free releases everything.
 *    Worst case per shard of N units and a caller capacity of C records, by
 *    the form a call takes (what a rank of a sharded text must be able to spare
 *    beside its text and its output; 8 GiB over 8 ranks: N = 2^29):
 *      AhoCorasick, tile kernel (the default)   20 C + 17 MB  (16-byte slots for
 *        1.25 C records + the waves' reservations)       C = N/128: 0.1 GB
 *      AhoCorasick, states form (texts with dense matches: 0.05 records per
 *        unit or more in the pool's last call)  4 N + N/128      N = 2^29: 2.0 GB
 *        -> without room: the tile kernel (nothing is launched before the
 *           buffers are there), also for the probe of a pool's first call
 *      AhoCorasick, DFA chunk scan              20 C
 *      LongestMatch, k_longest_bits             N/8 + N/1024      (marks, exits)
 *      LongestMatch, k_longest_follow           N/4 (+ 4 N for Map records)
 *      LongestMatch, walk pipeline              1.25 N .. 4.25 N  (lengths,
 *        block maxima, two bitmaps; states for Map records)
 *        -> a pool that cannot hold a form's buffers fails the call with
 *           ACGPU_E_NOMEM (the forms are not tried in turn)
 *      WholeWord                                6 N + 0.2 MB      (a 12-byte slot
 *        per two units)
 *        -> without room: 20 C + 17 MB (scratch slices + ordering pass)
 *      Shortest / WholeWordLongest              the AhoCorasick / WholeWord form
 *        + 16 bytes per record of the all-matches list / per walk start
 *    A cursor (acgpu_cursor_open below) needs the pool's scratch for ONE piece
 *    (N = its units + halo, at most cursor_max_piece = 2^26 + max_len + 1)
 *    plus buffers of its own:
 *      reservoir (device)                       up to cursor_reservoir_bytes
 *                                               (256 MiB): the piece's records
 *      page staging (pinned, device-mapped)     cap x record_kind of the
 *                                               largest page handed out
 *    A counting call (acgpu_count_* below) needs the pool's scratch for ONE piece as well, plus, kept by the pool:
 *      visit words (device)                     4 bytes per state of the compact automaton
 *      reservoir (device)                       up to cursor_reservoir_bytes: the Map records of a piece
 *                                               that is not counted directly
 *    A replace call (acgpu_replace_* below) needs the pool's scratch for ONE piece as well, plus, kept by the pool:
 *      reservoir (device)                       the counting calls' (up to cursor_reservoir_bytes): the Map records of a piece
 *      plan (device)                            8 bytes per record of the piece (+ 8 per 2048 records)
 *      replacement table (device)               8 bytes per replacement + 2 per replacement unit, uploaded per call
 *      slabs (device, the host entries)         2 x replace_slab_units x 2 bytes (2 x 64 MiB), or the result's size if smaller
 *    acgpu_replace_batch_u16 in addition, kept by the pool (N = the haystacks' units + one per haystack, H = the haystacks):
 *      concatenation (pinned, shared with       2.5 N + 5 H bytes
 *        acgpu_match_batch_u16)
 *      offsets (device)                         4 H in, 8 H out
 *      merged list (device)                     12 bytes per record and per separator of ONE piece, grow-only
 *      replacement table                        in its full form: 8 bytes per keyword given to acgpu_build (+ 8), whatever n_repl is
 *    acgpu_summary_batch_u16 needs the pool's scratch for ONE piece and the counting calls' reservoir as well, plus, kept by the
 *    pool (N and H as above):
 *      concatenation (pinned, shared with       2.5 N + 5 H bytes
 *        acgpu_match_batch_u16)
 *      offsets (device)                         4 H
 *      summaries (device)                       24 H, grow-only
 *    acgpu_count_batch_u16 needs the same without the summaries, plus, kept by the pool and grow-only:
 *      entry list (device)                      12 bytes per entry, at most cap entries
 *      staging (device)                         12 bytes per record of ONE piece (+ 12 per 2048 records)
 *    acgpu_match_utf8 needs what acgpu_match_u16 needs for the decoded text as ONE shard (N = its units, at most B, the bytes
 *    given: the staged text 2 N, the records cap x record_kind, the scan's form above), plus, kept by the pool:
 *      the bytes (device)                       B
 *      block sums (device)                      B/1024  (4 bytes per 4096 bytes)
 *      checkpoints (device)                     B/8 at most  (4 bytes per 32 units)
 *    acgpu_match_batch_utf8 / acgpu_summary_batch_utf8 need that for the span of B bytes and a staged text of N + H units (H = the
 *    haystacks, a separator unit behind each), plus, kept by the pool:
 *      byte offsets, haystacks' first units     4 H + 4 H (device)
 *      tagged records (match)                   cap x (record_kind + 4)
 *      summaries (summary)                      24 H, and the counting calls' reservoir
 *    The *_lossy forms of these three need the same, plus, kept by the pool:
 *      start bitmap (device)                    B/8, rounded up to 512 bytes per 4096  (a bit per byte)
 */
#ifndef ACGPU_H
#define ACGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACGPU_ABI_VERSION 5

/* error codes */
#define ACGPU_OK 0
#define ACGPU_E_INVALID (-1)     /* bad argument (NULL, misaligned device pointer, bad range ...)   */
#define ACGPU_E_NONWORD (-2)     /* java.lang.IllegalArgumentException of the WholeWord ctors:
                                    "<keyword> contains non-word characters."
                                    (S/WholeWordMatchMap.java:263-267, S/WholeWordMatchSet.java init) */
#define ACGPU_E_NOMEM (-3)       /* host or device allocation failed                                */
#define ACGPU_E_OVERFLOW (-4)    /* output capacity too small; *n_out holds the required record count */
#define ACGPU_E_HIP (-5)         /* HIP runtime error; see acgpu_last_hip_error()                    */
#define ACGPU_E_NODEVICE (-6)    /* no HIP device visible                                            */
#define ACGPU_E_UNSUPPORTED (-7) /* combination not implemented by this build                        */
#define ACGPU_E_ENCODING (-8)    /* the haystack is not well-formed UTF-8; stats->first_bad says where */

/* matcher families (which reference class an automaton replaces) */
#define ACGPU_MODE_ALL 0       /* AhoCorasickSet / AhoCorasickMap      S/AhoCorasickSet.java:193-252, S/AhoCorasickMap.java:277-336 */
#define ACGPU_MODE_LONGEST 1   /* LongestMatchSet / LongestMatchMap    S/LongestMatchSet.java:192-265, S/LongestMatchMap.java:288-360 */
#define ACGPU_MODE_WHOLEWORD 2 /* WholeWordMatchSet / WholeWordMatchMap S/WholeWordMatchSet.java:47-132, S/WholeWordMatchMap.java:155-240 */
#define ACGPU_MODE_SHORTEST 3  /* ShortestMatchSet / ShortestMatchMap   S/ShortestMatchSet.java:193-262, S/ShortestMatchMap.java:294-372;
                                  keyword_id = FIRST duplicate (S/ShortestMatchMap.java:47-49) */
#define ACGPU_MODE_WWLONGEST 4 /* WholeWordLongestMatchSet / Map        S/WholeWordLongestMatchSet.java:47-178, S/WholeWordLongestMatchMap.java:54-305;
                                  keywords are trimmed but may contain non-word characters */

/*
 * Word-character tables that are NOT fold-consistent (acgpu_info.fold_consistent == 0: a custom table, case-insensitive,
 * with wordChars[c] != wordChars[toLowerCase(c)] for some c).  The reference's loops differ in which lookups fold, and so
 * do the calls that replace them:
 *  - WholeWordMatchSet/Map.match(String) (S/WholeWordMatchMap.java:204,209 folded; :221,:226 raw) and
 *    WholeWordLongestMatchSet.match(String) (S/WholeWordLongestMatchSet.java:126 folded; :151,:156 raw) MIX folded and raw
 *    lookups, which makes token boundaries history dependent: acgpu_match_u16 / acgpu_match_device serve them with a
 *    sequential kernel over the whole haystack as ONE shard (own range = buffer, text_begin = text_end = 1;
 *    ACGPU_E_UNSUPPORTED for other shards).  For WWLONGEST that is the call with ACGPU_REC_SET.
 *  - WholeWordLongestMatchMap.match(String) (S/WholeWordLongestMatchMap.java:252,258,283,288: every lookup folded) -- the
 *    WWLONGEST call with ACGPU_REC_MAP -- and every match(Readable) loop (S/WholeWordMatchMap.java:112,117,328,
 *    S/WholeWordLongestMatchMap.java:404) -- acgpu_stream_feed -- fold in EVERY lookup: ordinary position-parallel scans
 *    over wordChars o toLowerCase; shards and streams as with a fold-consistent table.
 */

/* output record layouts */
#define ACGPU_REC_SET 8  /* acgpu_set_match: what SetMatchListener.match(haystack, start, end) receives */
#define ACGPU_REC_MAP 12 /* acgpu_map_match: MapMatchListener.match(haystack, start, end, value);
                            keyword_id indexes the caller's value array                             */

typedef struct acgpu_set_match {
    int32_t start, end;
} acgpu_set_match;

typedef struct acgpu_map_match {
    int32_t start, end;
    int32_t keyword_id; /* index (in the acgpu_build input) of the LAST keyword equal to the matched
                           (folded) string: reproduces "last value wins", S/AhoCorasickMap.java:49-50 */
} acgpu_map_match;

typedef struct acgpu_automaton acgpu_automaton;

/*
 * Replaces the constructors: AhoCorasickSet(Iterable<String>, boolean[, Thresholder])
 * S/AhoCorasickSet.java:16-191, AhoCorasickMap(...) S/AhoCorasickMap.java:20-206,
 * LongestMatchSet(...) S/LongestMatchSet.java:15-190, WholeWordMatchMap/Set(...) + init
 * S/WholeWordMatchMap.java:21-53,246-323.
 *
 *  kw_units/kw_off : keyword i is kw_units[kw_off[i] .. kw_off[i+1]).  A null or empty Java
 *                    keyword is an empty range (both are skipped, S/AhoCorasickSet.java:27).
 *  case_sensitive  : 0 => every keyword unit and haystack unit is mapped through lower_tbl
 *                    (Character.toLowerCase(char), S/AhoCorasickSet.java:33,229).
 *  lower_tbl       : 65536 entries, required when case_sensitive == 0 (the caller's JVM fills
 *                    it with its own Character.toLowerCase so that parity holds for that JVM).
 *  wordchar_tbl    : 65536 flags, required for ACGPU_MODE_WHOLEWORD and ACGPU_MODE_WWLONGEST
 *                    (WordCharacters.generateWordCharsFlags*, S/WordCharacters.java:6-39).
 *  bad_keyword     : on ACGPU_E_NONWORD receives the index of the offending keyword (may be NULL).
 * The Thresholder argument of the reference constructors is a results-neutral memory/speed
 * knob of its node representation and has no counterpart here.
 */
int acgpu_build(int mode, const uint16_t *kw_units, const uint64_t *kw_off, uint32_t n_kw, int case_sensitive,
                const uint16_t *lower_tbl, const uint8_t *wordchar_tbl, acgpu_automaton **out, int64_t *bad_keyword);

void acgpu_free(acgpu_automaton *a);

typedef struct acgpu_info {
    uint32_t abi_version;
    uint32_t mode;
    uint32_t case_sensitive;
    uint32_t n_states;       /* trie nodes incl. root                                   */
    uint32_t n_classes;      /* character classes incl. class 0 = "in no keyword"       */
    uint32_t n_keywords;     /* distinct non-empty (folded, trimmed) keywords           */
    uint32_t min_keyword_len;
    uint32_t max_keyword_len;
    uint32_t dense;          /* 1: dense state x class table, 0: hashed edges + fail links */
    uint32_t entry_bytes;    /* 2 or 4                                                   */
    uint64_t table_bytes;    /* bytes of the transition structure resident in HBM        */
    uint32_t lds_states;     /* states whose rows are staged in LDS by the scan kernel   */
    uint32_t fold_consistent;/* WHOLEWORD / WWLONGEST: wordchar[c] == wordchar[lower[c]] for all c (see above) */
    uint32_t filter_k;       /* ALL: length of the suffix K-gram filter, 0 = none          */
    uint32_t filter_bits;    /* ALL: size of the K-gram bitmap in bits                      */
    uint32_t tile_kernel;    /* ALL/SHORTEST: 1 if the position-parallel K-gram kernel will be used (whenever the filter
                                exists); LONGEST: 1 if the filter is selective (all-matches pipeline + selection) */
    float filter_density;    /* ALL: fraction of K-grams (over keyword units) that pass     */
    uint32_t fold_clean;     /* WHOLEWORD: every FOLDED keyword unit is a word character (always 1 with a fold-consistent
                                table: keywords are validated on their raw units, S/WholeWordMatchMap.java:263-267); 0: a
                                folding scan walks the keyword trie through units it does not take for word characters */
} acgpu_info;

int acgpu_get_info(const acgpu_automaton *a, acgpu_info *info);

/*
 * Replaces StringSet.match(String, SetMatchListener) / StringMap.match(String, MapMatchListener)
 * for a haystack in HOST memory: copies it to the current HIP device, scans, and returns every
 * record the reference would have passed to its listener, in the reference's call order
 * (ALL: end ascending then start ascending, S/AhoCorasickSet.java:522-535; LONGEST and
 * WHOLEWORD: position order).  The facade then runs the listener loop itself, stopping at the
 * first `false` -- observationally identical to the reference's early stop
 * (S/AhoCorasickSet.java:223-225).
 *  record_kind : ACGPU_REC_SET or ACGPU_REC_MAP (layout of `out`).
 *  cap         : capacity of `out` in records.  On ACGPU_E_OVERFLOW nothing useful is in `out`
 *                and *n_out is the capacity to retry with.
 *  n_units     : < 2^31 (Java String limit).
 */
int acgpu_match_u16(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, int record_kind, void *out,
                    uint64_t cap, uint64_t *n_out);

/*
 * Many short haystacks in ONE call (the reference publishes one workload: a paragraph against a 235 k-word dictionary at
 * 3.6 us per match() call, R/README.md:130-148; a call here has tens of microseconds of fixed cost, so short inputs are
 * batched): haystack i is units[offsets[i] .. offsets[i+1]).  The haystacks are scanned as one text with a separator unit
 * between them that no keyword contains (word matchers: and that is no word character), so every haystack's matches are
 * exactly what match(String) reports for it alone -- any family.  Records carry the haystack index in front:
 *   ACGPU_REC_SET -> acgpu_batch_set_match {haystack, start, end}, ACGPU_REC_MAP -> acgpu_batch_map_match {haystack, start,
 *   end, keyword_id}; positions are relative to their haystack; order: haystack ascending, inside a haystack the
 *   reference's listener-call order.  The facade calls the listener per record and, if it returns false, skips the rest of
 *   THAT haystack's records.
 * WholeWordLongest: the reference's scan starts a walk at position 0 whatever stands there (and a keyword without word
 * characters gives the root a transition on a non-word unit), so the unit behind every separator is a walk start too.
 * One call per haystack inside the library instead, same results: a dictionary that uses all 65536 units, and the word
 * matchers over a table that is not fold-consistent (acgpu_info.fold_consistent == 0).
 * offsets[n_haystacks] - offsets[0] + n_haystacks must stay below 2^31.  On ACGPU_E_OVERFLOW *n_out is the capacity to retry with.
 */
typedef struct acgpu_batch_set_match {
    int32_t haystack, start, end;
} acgpu_batch_set_match;
typedef struct acgpu_batch_map_match {
    int32_t haystack, start, end, keyword_id;
} acgpu_batch_map_match;
int acgpu_match_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                          int record_kind, void *out, uint64_t cap, uint64_t *n_out);

/*
 * Device-resident form of the same call, and the unit of multi-GPU sharding.
 * The buffer holds an owned range plus halos; positions in the records are relative to the
 * buffer start.  Ownership: ALL -> a match belongs to the shard that owns its LAST unit (left
 * halo >= max_keyword_len-1 units needed); WHOLEWORD -> to the shard that owns the first unit of
 * the word (left halo 1 unit, right halo up to the end of the word or max_keyword_len+1 units);
 * LONGEST -> to the shard that owns its first unit, given the greedy chain's entry position
 * (right halo >= max_keyword_len-1 units); WWLONGEST -> to the shard that owns its first unit (left halo 1 unit, right
 * halo max_keyword_len+1 units), given the position from which the scan looks for its next word start (chain_entry;
 * chain_exit: a position behind the last walk this shard's scan made from which the search for the next word start finds
 * what the reference's scan finds -- behind the walk's stop, or behind the word in which the walk died); SHORTEST -> to the shard that owns its LAST unit (left halo as ALL), given
 * the position at which matching last restarted (chain_entry: no match may start before it; chain_exit: the end of
 * the last match reported, or chain_entry if there was none).
 */
typedef struct acgpu_shard {
    const uint16_t *d_hay; /* device pointer, 16-byte aligned                                   */
    uint64_t n_units;      /* units in the buffer, < 2^31                                        */
    uint64_t own_begin;    /* owned range [own_begin, own_end) inside the buffer                 */
    uint64_t own_end;
    int32_t text_begin;    /* 1: buffer unit 0 is the first unit of the whole haystack           */
    int32_t text_end;      /* 1: buffer unit n_units-1 is the last unit of the whole haystack    */
    int64_t chain_entry;   /* LONGEST in : first greedy-chain position >= own_begin (own_begin on the first shard);
                              WWLONGEST in: the scan visits the first word start at or after this position;
                              SHORTEST in: position of the last restart (0 on the first shard)      */
    int64_t chain_exit;    /* LONGEST out: first greedy-chain position >= own_end; WWLONGEST / SHORTEST out: see above */
    void *d_result;        /* optional device pointer (16-byte aligned) to an acgpu_device_result that the call's last
                              kernel (or a copy enqueued behind it) fills in STREAM ORDER: a multi-GPU driver points it
                              into the buffer it all-gathers, so the record count travels with the records and no host
                              round trip sits between the scan and the collective.  NULL: not wanted.            */
} acgpu_shard;

/* what acgpu_shard.d_result receives */
typedef struct acgpu_device_result {
    uint64_t n_records; /* records the call produced (may exceed cap: then d_out is incomplete)                     */
    uint32_t redone;    /* non-zero: the library has to redo this call (acgpu_match_device_end does) -- the records
                           behind this header are not valid yet; a driver that gathered them gathers again          */
    uint32_t reserved;
} acgpu_device_result;

/* optional per-call timing of the device work, measured with HIP events on `stream` */
typedef struct acgpu_profile {
    float scan_ms;     /* the dominant kernel: one pass over the haystack units                  */
    float finalize_ms; /* ordering of records (prefix sum of per-chunk counts + permutation)     */
    float total_ms;    /* first launch to last launch of the call                                */
    uint64_t scan_units;   /* haystack units the scan kernel processed (owned + halo)            */
    uint64_t n_matches;
    char scan_kernel[64];  /* name of the dominant kernel as it appears in rocprofv3             */
} acgpu_profile;

/*
 *  d_out  : device pointer to cap records of record_kind (16-byte aligned).
 *  stream : hipStream_t (NULL = the default stream).  The call enqueues its kernels on `stream`
 *           and synchronises that stream once, to read back the record count.
 *  prof   : NULL, or receives HIP-event timings of this call.
 */
int acgpu_match_device(const acgpu_automaton *a, acgpu_shard *shard, int record_kind, void *d_out, uint64_t cap,
                       uint64_t *n_out, void *stream, acgpu_profile *prof);

/*
 * Asynchronous form: _begin enqueues the whole pipeline on `stream` and returns without waiting; _end waits for that call only
 * (an event, not the stream) and returns its count / timings.  Up to 4 calls may be in flight per automaton and device.
 * Lets a host keep the GPU busy across calls: the next scan is queued while the previous count travels back.
 * want_profile != 0 records the HIP events that _end turns into acgpu_profile.
 * The acgpu_shard passed to _begin must stay alive until _end (or _abandon) has returned: _end writes chain_exit into it.
 *  - Enqueued without any host round trip: ACGPU_MODE_ALL, ACGPU_MODE_WHOLEWORD (fold-consistent tables) and
 *    ACGPU_MODE_LONGEST through its walk pipeline (shard->chain_entry is read at _begin; chain_exit is written to the
 *    SAME acgpu_shard object when _end returns, so it must outlive the ticket).
 *  - The other families (and LONGEST over a dictionary with a selective suffix filter, whose sparse form decides on the
 *    host) run inside _begin: the ticket is complete when _begin returns and _end only hands the result over.
 *
 *  - ACGPU_MODE_ALL chooses between the tile kernel and the states form by what the pool's LAST call found (records per
 *    unit).  A pool's first call asks the text itself -- the first 2^20 units are counted first -- only when it is
 *    synchronous and the text has 2^23 units or more: a first call through _begin, or on a shorter text, takes the tile
 *    kernel.  The records are the same either way; on a word list in natural text the first enqueued call is the slow one.
 *
 * STREAM RULE.  All calls on one automaton and device share that automaton's scratch pool; stream order is what keeps
 * them apart.  While tickets are in flight, EVERY call on that automaton and device -- another _begin, a synchronous
 * acgpu_match_device, acgpu_match_u16 or acgpu_stream_feed (both use the NULL stream) -- must use the stream of the
 * tickets; a call on a different stream is refused with ACGPU_E_INVALID instead of racing on the scratch.  With no
 * ticket in flight any stream may be used (a synchronous call has left the scratch idle when it returns).
 */
typedef struct acgpu_ticket acgpu_ticket;
int acgpu_match_device_begin(const acgpu_automaton *a, acgpu_shard *shard, int record_kind, void *d_out, uint64_t cap,
                             void *stream, int want_profile, acgpu_ticket **ticket);
int acgpu_match_device_end(const acgpu_automaton *a, acgpu_ticket *ticket, uint64_t *n_out, acgpu_profile *prof);
/* Gives a ticket up without collecting it: waits until its kernels have finished (they write the caller's buffers until
 * then), never redoes the call.  For a driver that already knows -- from the device result it gathered -- that the step has
 * to be done again with larger buffers. */
int acgpu_match_device_abandon(const acgpu_automaton *a, acgpu_ticket *ticket);

/*
 * ---- several devices, ONE host process -------------------------------------------------------------------------------------
 * BASELINE north_star: "long haystacks shard naturally across the 8 GPUs of one node with an RCCL all-gather over xGMI of
 * per-shard match buffers plus a (longest-pattern - 1) halo".  The reference's call is one call in one process
 * (S/StringSet.java:3-5, S/StringMap.java:5-9: match(String haystack, listener)); so is this one.
 *
 * acgpu_match_u16_multi: acgpu_match_u16 with the haystack cut into n_devices contiguous shares, share i on HIP device
 * devices[i] -- each with its own pinned staging ring, copy stream, scan stream and copy of the automaton's tables, each fed
 * and scanned by its own host thread, all at once.  A share carries the halo its family needs (ALL / SHORTEST: max_len-1
 * units on the left; WHOLEWORD / WWLONGEST: 1 unit on the left, max_len+1 on the right; LONGEST: max_len-1 on the right).
 * The chain families (LONGEST, SHORTEST, WWLONGEST) scan every share speculatively and repair the head of a share whose
 * true entry -- the previous share's exit -- differs (two short window scans, as a rule).  Records arrive in `out` in the
 * reference's listener-call order for the WHOLE haystack with global positions: exactly what acgpu_match_u16 returns.
 *  devices   : n_devices HIP device ordinals.  A device may be named more than once (further shares on the same device get
 *              their own scratch pool and stream): how a one-GPU box tests the split.
 *  A share has fixed costs (a host thread, a pinned staging ring, two synchronisations), so a haystack is cut into at most
 *  n_units / 2^22 shares (8 MiB of text each; development tunable "multi_min_share"); shorter ones, and the loops that only
 *  exist as one sequential scan (word matchers over a table that is not fold-consistent), run on devices[0] alone through
 *  acgpu_match_u16.
 *  Scaling: every share is fed from the CALLER's memory by host threads copying pageable -> pinned memory (about 45 GB/s per
 *  share on one socket), so this entry is bound by the host's copy bandwidth beyond about two devices per socket; the feeder
 *  threads of a share are pinned to the NUMA node of its device where the platform reports one.  The form that scales with the
 *  device count is acgpu_match_device_allgather below: shards resident in device memory, nothing of the text on the host.
 * The calling thread's current device is restored.  Errors and ACGPU_E_OVERFLOW as acgpu_match_u16.
 */
int acgpu_match_u16_multi(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, const int *devices, int n_devices,
                          int record_kind, void *out, uint64_t cap, uint64_t *n_out);

/*
 * Device-resident form with the gather the north_star names: every device scans ITS shard (already in its memory, halos in
 * place: acgpu_shard as for acgpu_match_device) into its own slot of a gather buffer, and one all-gather leaves every
 * device with every shard's records -- config 3 of BASELINE.json.
 *
 * acgpu_comm: the devices of a job, one stream per device, and the transport of the gather:
 *   ACGPU_TRANSPORT_RCCL : single-process RCCL (ncclCommInitAll over the device list, one ncclAllGather per device inside
 *                          ncclGroupStart/End, in place).  librccl.so.1 is bound at run time (dlopen): libacgpu.so does not
 *                          link it, and ACGPU_E_UNSUPPORTED is returned where it is missing.  Needs distinct devices.
 *   ACGPU_TRANSPORT_PEER : hipMemcpyPeerAsync of every slot to every other device over the direct xGMI links (also what a
 *                          device list that names a device twice gets).
 *   ACGPU_TRANSPORT_AUTO : RCCL when the devices are distinct and the library loads, else peer copies.
 *
 * Gather buffer of device i: n_devices slots of acgpu_gather_slot_bytes(gcap, record_kind) bytes; slot j =
 * [the 16 bytes of an acgpu_device_result | gcap records] of shard j, positions relative to shard j's buffer.  d_gather[i] is a
 * device pointer on devices[i], 16-byte aligned.
 *  shards  : n_devices shards, shard i resident on devices[i].  Chain families: shards[0].chain_entry is the chain's entry
 *            into the whole text; every shards[i].chain_exit is set to the true scan's exit from shard i.
 *  counts  : receives the n_devices record counts (also in the gathered headers).
 *  profs   : NULL, or n_devices acgpu_profile structs: HIP-event timings of each device's scan.
 * Returns ACGPU_E_OVERFLOW when some count exceeds gcap: counts[] are exact, the buffers hold nothing useful, nothing was
 * gathered; call again with gcap >= the largest count.
 * AhoCorasick and WholeWord (fold-consistent tables) are enqueued on every device without a host round trip (scan, header
 * and gather in stream order; one host wait at the end); the other families run their shards on one host thread per
 * device, then the repairs, then the gather.
 */
#define ACGPU_TRANSPORT_AUTO 0
#define ACGPU_TRANSPORT_RCCL 1
#define ACGPU_TRANSPORT_PEER 2
typedef struct acgpu_comm acgpu_comm;
int acgpu_comm_open(const int *devices, int n_devices, int transport, acgpu_comm **out);
void acgpu_comm_close(acgpu_comm *c);
int acgpu_comm_transport(const acgpu_comm *c);       /* the transport in use: ACGPU_TRANSPORT_RCCL or _PEER              */
void *acgpu_comm_stream(const acgpu_comm *c, int i); /* hipStream_t of device i: work a caller enqueues there (filling the
                                                        shard, reading the gathered records) is ordered with the call's   */
uint64_t acgpu_gather_slot_bytes(uint64_t gcap, int record_kind); /* (16 + gcap * record_kind), rounded up to 16 */
int acgpu_match_device_allgather(const acgpu_automaton *a, acgpu_comm *c, acgpu_shard *shards, int record_kind,
                                 void *const *d_gather, uint64_t gcap, uint64_t *counts, acgpu_profile *profs);
int acgpu_last_rccl_error(void); /* ncclResult_t of the last RCCL failure on this thread */

/*
 * Replaces StringMap.match(Readable, ReadableMatchListener<T>) (S/StringMap.java:6; S/AhoCorasickMap.java:208-275,
 * S/LongestMatchMap.java:203-286, S/WholeWordMatchMap.java:55-153): the haystack arrives in chunks of any size (the
 * reference reads it through a CharBuffer) and may be longer than a Java String.  Every feed returns the records that
 * have become decidable, in the reference's call order; the concatenation over all feeds is what match(String) would
 * deliver for the whole text (T/MapTest.java:178-188).  The facade passes record.keyword_id -> value to the listener
 * (the Readable listener receives only the value) and may stop feeding when the listener returns false.
 *  feed   : units = the next n_units of the haystack in HOST memory (may be 0); final != 0 marks the end of the
 *           haystack, after which only close is valid.  Internally the stream keeps the few units a later chunk can
 *           still change the answer for (ALL: max_keyword_len-1 units of left context; WHOLEWORD: one unit of context
 *           plus the last max_keyword_len+1 units, whose words are decided by the next feed; LONGEST: the last
 *           max_keyword_len-1 units plus the position at which the greedy chain continues; WWLONGEST: as WHOLEWORD plus
 *           the position from which the scan looks for its next word start).
 *  out    : cap records of record_kind; start/end are int32 relative to *base (the global position, in units since
 *           the first feed, that record coordinate 0 stands for).  On ACGPU_E_OVERFLOW nothing was consumed: *n_out
 *           is the capacity to call the SAME feed again with.
 *  carried units + n_units must stay below 2^31.
 *  Word-character tables that are not fold-consistent: the Readable loops fold in every lookup (see above), and so do
 *  the feeds.
 *  Lifetime and device: close a stream BEFORE acgpu_free of its automaton (one that is still open then is detached: its
 *  feeds return ACGPU_E_INVALID, acgpu_stream_close stays safe).  Every feed and acgpu_stream_reserve must come from a
 *  thread whose current HIP device is the one of the stream's first feed: another device returns ACGPU_E_INVALID.
 */
typedef struct acgpu_stream acgpu_stream;
int acgpu_stream_open(const acgpu_automaton *a, acgpu_stream **out);
int acgpu_stream_feed(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, int record_kind, void *out,
                      uint64_t cap, uint64_t *n_out, int64_t *base);
void acgpu_stream_close(acgpu_stream *s);
/*
 * The pipelined form of the feeds (call before the first feed; on != 0).  A feed then copies its chunk into pinned staging
 * memory with several host threads -- every piece goes on its way to the device as soon as it has been copied -- while the
 * calling thread scans the PREVIOUS chunk and returns ITS records: host copy, transfer and scan of neighbouring chunks
 * overlap.  Differences to the default form, all of them about WHEN records arrive, none about which:
 *  - a feed returns the records the previous feed's chunk made decidable (the first feed returns none); the feed with
 *    final != 0 returns the previous chunk's and its own; *base is the position record coordinate 0 stands for, as before;
 *  - ACGPU_E_OVERFLOW: the chunk HAS been consumed; call the same feed again with the capacity in *n_out and it hands the
 *    records over (its units are not looked at again);
 *  - carried units + n_units must stay below 2^30; all feeds of a stream come from threads whose current HIP device is the
 *    one the first feed ran on.
 * acgpu_stream_reserve (pipelined streams): the address at which the next chunk of up to n_units units may be WRITTEN by the
 * caller -- the staging memory itself; a feed whose `units` is that address copies nothing (a JNI glue reads the Java char[]
 * straight into it).
 */
int acgpu_stream_set_pipelined(acgpu_stream *s, int on);
int acgpu_stream_reserve(acgpu_stream *s, uint64_t n_units, uint16_t **buf);

/*
 * Cursor over ONE match(String, listener) call: the records acgpu_match_u16 would return for the haystack, handed out in the
 * reference's listener-call order in pages of a size the caller chooses, and scanned only as far as the pages taken so far
 * require -- a listener that returns false stops the scan where the reference stops (S/AhoCorasickSet.java:223-225), and a text
 * with more records than one buffer (or one Java int[]) holds is drained page by page.
 *  open  : haystack in HOST memory, n_units < 2^31; the caller keeps it alive and unchanged until close.  record_kind as for
 *          acgpu_match_u16.  The cursor's device is the current HIP device at open (the automaton's tables are uploaded there
 *          then: without a device, open fails as acgpu_match_u16 does).
 *  next  : copies the next 1 .. cap records (cap >= 1) into `out` (record_kind layout, positions in haystack coordinates) and
 *          returns ACGPU_OK; *n_out == 0 with ACGPU_OK: every record has been handed out.  Never ACGPU_E_OVERFLOW.  The
 *          concatenation of all pages is, record for record, what acgpu_match_u16 returns for the same haystack and record_kind
 *          (every family, both record kinds, fold-consistent word tables or not).
 *  stats : progress of the scan, see acgpu_cursor_stats.
 * How it scans: the owned units are cut into PIECES, each scanned by itself with the halo its family needs (as a share of
 * acgpu_match_u16_multi carries) and the chain handed on from the piece before -- pieces run in sequence, so nothing is
 * repaired.  The first piece has "cursor_first_piece" units (default 2^20), every further one four times the one before, up to
 * "cursor_max_piece" (2^26), and never more than the records seen per unit so far predict to fill half of the reservoir: a
 * device buffer of the cursor's own that holds the records of the current piece and grows up to "cursor_reservoir_bytes"
 * (256 MiB).  A piece whose records do not fit is scanned again -- in a larger reservoir, or shrunk -- and counted in
 * `rescans`.  A unit holds at most max_keyword_len records (ALL / SHORTEST) or one (the others), so a piece of one unit always
 * fits a reservoir of that many records; ACGPU_E_NOMEM only where even that does not.  The loops that exist only as one
 * sequential scan (word matchers over a table that is not fold-consistent, see above) scan the whole text as one piece.
 * A next whose reservoir is empty scans pieces until one yields a record or the text ends; nothing is scanned ahead while the
 * caller holds a page.
 * Device and lifetime as for acgpu_stream_*: next from a thread whose current device is not the cursor's returns
 * ACGPU_E_INVALID; close a cursor before acgpu_free of its automaton (one still open then is detached: next returns
 * ACGPU_E_INVALID, close stays safe); tickets in flight on the automaton and device make next return ACGPU_E_INVALID.
 * One thread at a time per cursor.  Other cursors and match calls on the same automaton may run between page calls: the scratch
 * pool is held only inside next.  After a next that failed, only close is valid.
 * Memory, besides the pool's scratch for one piece (its units plus halo, and the scan's buffers for them): the reservoir (up to
 * cursor_reservoir_bytes of device memory) and a pinned, device-mapped page staging buffer of the largest page handed out.
 */
typedef struct acgpu_cursor acgpu_cursor;
typedef struct acgpu_cursor_stats {
    uint64_t records_delivered; /* handed out by the page calls so far                                   */
    uint64_t records_buffered;  /* scanned, not yet handed out (held in the cursor's device reservoir)   */
    uint64_t units_scanned;     /* owned haystack units scanned so far, rescans included                  */
    uint64_t scan_end;          /* haystack units [0, scan_end) have been scanned                         */
    uint32_t pieces, rescans;   /* piece scans; of those, scans repeated because the reservoir overflowed */
    uint32_t done;              /* 1: text exhausted and every record handed out                          */
    uint32_t reserved;
} acgpu_cursor_stats;
int acgpu_cursor_open(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, int record_kind,
                      acgpu_cursor **out);
int acgpu_cursor_next(acgpu_cursor *c, void *out, uint64_t cap, uint64_t *n_out);
int acgpu_cursor_get_stats(const acgpu_cursor *c, acgpu_cursor_stats *st);
void acgpu_cursor_close(acgpu_cursor *c);

/*
 * Counting: how often every keyword occurs -- what a listener that does nothing but counts[value]++ would hold -- without a
 * record being handed out.  counts[i] = the number of records with keyword_id == i that acgpu_match_u16 / acgpu_match_device
 * with ACGPU_REC_MAP would return for the same automaton, text and shard: every family, the word matchers over tables that are
 * not fold-consistent included; ids as in the Map records: the LAST duplicate of a keyword is counted, for Shortest the FIRST;
 * the slots of empty keywords and of the other duplicates stay 0.
 *  n_counts : the number of keywords given to acgpu_build (else ACGPU_E_INVALID).
 *  acgpu_count_u16    : haystack in HOST memory, n_units < 2^31; OVERWRITES the host array counts[n_counts].  Without a device
 *                       it fails as acgpu_match_u16 does and leaves counts untouched.
 *  acgpu_count_device : the shard as for acgpu_match_device (halos, text_begin / text_end, chain_entry in, chain_exit out;
 *                       d_result is not written); ADDS to the device array d_counts[n_counts] (8-byte aligned), which the caller
 *                       zeroes -- shards, ranks and steps accumulate into one array (AhoCorasick and WholeWord counts are
 *                       additive over the shards of a text; the chain families hand chain_exit on to the next shard's
 *                       chain_entry).  Synchronous: everything is enqueued on `stream`; the call waits for that stream
 *                       once per piece (for the piece's record count, as acgpu_match_device does) and once at the end.  The
 *                       STREAM RULE above applies (tickets in flight on another stream: ACGPU_E_INVALID, nothing is added).
 *                       After any other error d_counts is undefined (pieces already counted have been added, visit tallies of
 *                       direct pieces have not): zero it before the next use.
 *  st       : NULL, or receives how the text was counted.
 * Errors as for the match calls; never ACGPU_E_OVERFLOW (there is no caller capacity).
 * How it counts: the owned units are cut into pieces as a cursor's are (the same ramp -- cursor_first_piece, x 4,
 * cursor_max_piece -- density cap and rescan rules; the chain handed on from piece to piece), and a piece is counted
 *  - directly (ACGPU_MODE_ALL, where a record call would take the states form -- dense matches, a compact automaton): the
 *    automaton's state behind every owned unit is tallied per state (4-byte visit words), and after the last piece every
 *    visited state's tally is added to each keyword that ends in it.  No record is written, ordered or copied;
 *  - or through Map records in a device reservoir of the call's own, whose keyword_id column is added to the counts on the
 *    device.  Records that do not fit the reservoir: the piece is scanned again (st->rescans), larger reservoir or smaller piece.
 * A counting call teaches the pool its density as a record call does: on a word list in natural text the first piece goes
 * through records, the following ones are counted directly.
 * Memory, besides the pool's scratch for one piece: the visit words (4 bytes per state of the compact automaton; without
 * room for them every piece goes through records), a reservoir of at most cursor_reservoir_bytes (kept by the pool, grow-only),
 * and for acgpu_count_u16 the counts on the device (8 bytes per keyword).
 */
typedef struct acgpu_count_stats {
    uint64_t n_records;     /* records the equivalent Map match call would have returned == what this call added to counts[] in total */
    uint64_t units_direct;  /* owned units counted from the automaton's states: no record written                                      */
    uint64_t units_records; /* owned units counted through Map records in the call's own device reservoir                              */
    uint32_t pieces, rescans; /* pieces: scan attempts (a host text's piece may be several shard calls); rescans: of those, attempts
                                 that ended at a shard whose records did not fit -- the shards in front of it stay counted, the rest
                                 of the piece is scanned again                                                                      */
} acgpu_count_stats;
int acgpu_count_u16(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, uint64_t *counts, uint32_t n_counts,
                    acgpu_count_stats *st);
int acgpu_count_device(const acgpu_automaton *a, acgpu_shard *shard, uint64_t *d_counts, uint32_t n_counts, void *stream,
                       acgpu_count_stats *st);

/*
 * Replace: the text with every match substituted -- what a listener doing sb.append(haystack, last, start).append(value);
 * last = end would build -- written on the device; no record reaches the host.  With r_0 .. r_{k-1} the Map records
 * acgpu_match_u16 returns for the same automaton and text, in their order, and e_{-1} = 0, the result is
 *   hay[e_{-1}:s_0] + repl[id_0] + hay[e_0:s_1] + repl[id_1] + ... + hay[e_{k-1}:n]
 * for the four families whose records never overlap and come in position order: ACGPU_MODE_LONGEST, _SHORTEST, _WHOLEWORD,
 * _WWLONGEST (word tables that are not fold-consistent included).  ACGPU_MODE_ALL: ACGPU_E_UNSUPPORTED, before any device is
 * touched (its records overlap, and the listener order does not say which one wins).
 *  repl_units / repl_off : HOST arrays in the layout of kw_units / kw_off: replacement i is repl_units[repl_off[i] .. repl_off[i+1]),
 *              indexed by keyword_id exactly as a Map value array is (the LAST duplicate's slot is the one read, for Shortest the
 *              FIRST; the slots of empty keywords and of the other duplicates are never read).  An empty replacement deletes the
 *              match.  A case-insensitive automaton replaces whatever case matched.
 *  n_repl    : the number of keywords given to acgpu_build, or 1: that one replacement stands for every keyword (masking).
 *              Anything else, or more than 2^31 replacement units in all: ACGPU_E_INVALID.
 *  cap, *n_out : in UNITS.  A result of more than cap units: ACGPU_E_OVERFLOW with *n_out (and st->units_out) the exact size;
 *              out[0 .. cap) is then unspecified and nothing at or beyond cap has been written (the rest of the text is still
 *              scanned and planned, for the size, but neither emitted nor copied).  *n_out may exceed 2^32.
 *  acgpu_replace_u16    : haystack in HOST memory, n_units < 2^31; `out` is host memory.  Without a device it fails as
 *              acgpu_match_u16 does and leaves `out` untouched.  Works on the NULL stream (STREAM RULE above), under the pool's lock.
 *  acgpu_replace_device : the shard must be a WHOLE text (own_begin == 0, own_end == n_units, text_begin == text_end == 1), else
 *              ACGPU_E_UNSUPPORTED: rewriting one shard of a sharded text needs the position up to which the rank before it has
 *              emitted handed on between the ranks, which is not built (nor is a multi-device form; a text in chunks:
 *              acgpu_stream_replace_u16 below).  d_out:
 *              device memory, 16-byte aligned, written directly (clipped at cap).  Everything is enqueued on `stream`; the call
 *              waits for it per piece -- for the piece's record count, as acgpu_count_device does, and for its output length -- and
 *              once at the end.
 * How it works: the text is cut into pieces as a cursor's are (the same ramp and rescan rules); a piece's Map records go to the
 * pool's reservoir; a prefix sum over them (the plan) gives every replacement its output position, and one kernel writes the
 * piece's part of the result from the text and the replacement table, for the host entry slab by slab ("replace_slab_units",
 * default 2^25 units: a slab is copied out while the next is written).  A piece emits the text up to a position before which no
 * later record can start: for the families whose match belongs to the piece that owns its first unit, the end of its owned range
 * or of its last record; for Shortest, max_keyword_len - 1 units less than that (emitted from the next piece's left halo).
 */
typedef struct acgpu_replace_stats {
    uint64_t n_records;       /* matches replaced == records the Map match call returns                      */
    uint64_t units_out;       /* units of the rewritten text (exact, also on ACGPU_E_OVERFLOW)               */
    uint32_t pieces, rescans; /* as acgpu_count_stats                                                        */
} acgpu_replace_stats;
int acgpu_replace_u16(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, const uint16_t *repl_units,
                      const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap, uint64_t *n_out,
                      acgpu_replace_stats *st);
int acgpu_replace_device(const acgpu_automaton *a, acgpu_shard *shard, const uint16_t *repl_units, const uint64_t *repl_off,
                         uint32_t n_repl, uint16_t *d_out, uint64_t cap, uint64_t *n_out, void *stream, acgpu_replace_stats *st);

/*
 * Many short texts rewritten in ONE call (a replace call has the fixed cost of a match call, a table upload and its waits on
 * top): haystack i is units[offsets[i] .. offsets[i+1]) as for acgpu_match_batch_u16, empty ones allowed, and the result is
 * out[out_offsets[i] .. out_offsets[i+1]), unit for unit what acgpu_replace_u16 returns for haystack i alone.  The results lie
 * back to back, no separator between them; out_offsets has n_haystacks + 1 entries, out_offsets[0] == 0 and
 * *n_out == out_offsets[n_haystacks].  repl_units / repl_off / n_repl, cap and *n_out: as for acgpu_replace_u16.
 *  st        : n_records is the sum over the haystacks, units_out == *n_out; pieces and rescans are those of the one text the
 *              haystacks are scanned as (of the calls per haystack, summed, where the library makes those).
 *  errors    : ACGPU_E_UNSUPPORTED for ACGPU_MODE_ALL, before any device is touched.  ACGPU_E_INVALID: NULL offsets, n_out or
 *              out_offsets; descending offsets; a bad replacement table; offsets[n_haystacks] - offsets[0] + n_haystacks >= 2^31;
 *              tickets in flight on the pool (the call works on the NULL stream, under the pool's lock, as the batch match call).
 *              n_haystacks == 0: ACGPU_OK, *n_out = 0, out_offsets[0] = 0, no device needed.
 *  overflow  : a result of more than cap units gives ACGPU_E_OVERFLOW; *n_out and EVERY entry of out_offsets are exact all the
 *              same (the plan runs to the end), and nothing at or beyond out[cap] has been written.
 * How it works: the haystacks are concatenated with a separator unit behind each, as acgpu_match_batch_u16 does, and that text
 * goes through the pieces of acgpu_replace_u16 -- with a separator treated as a match that is deleted: behind every piece its
 * records are merged with the pseudo-records of its separators (k_replace_merge), plan and emit run over the merged list
 * unchanged, and the plan's position of a separator is where the next haystack's result begins (k_replace_batch_offsets).  One
 * scan, one plan and one emit, no second pass over the output; the waits per piece are those of acgpu_replace_u16.
 * One acgpu_replace_u16 call per haystack inside the library instead, same results, where acgpu_match_batch_u16 falls back: a
 * dictionary that uses all 65536 units, and the word matchers over a table that is not fold-consistent.
 * No device-resident or multi-device form of this call exists, nor a stream of batches (one long text in chunks:
 * acgpu_stream_replace_u16 below).
 */
int acgpu_replace_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                            const uint16_t *repl_units, const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap,
                            uint64_t *out_offsets /* n_haystacks + 1 */, uint64_t *n_out, acgpu_replace_stats *st);

/*
 * Many short texts DECIDED in one call: for every haystack how many records it has and the first of them -- what a listener that
 * returns false from its first call, or one that only counts, would hold -- reduced on the device; no record reaches the host.
 * Haystack i is units[offsets[i] .. offsets[i+1]) as for acgpu_match_batch_u16, empty ones allowed.  out[i] is {count, first
 * record} of the records with haystack == i that acgpu_match_batch_u16(..., ACGPU_REC_MAP, ...) returns for the same arguments:
 * every family, ACGPU_MODE_ALL included (nothing here needs records that do not overlap); positions relative to the haystack,
 * keyword_id as in a Map record (the LAST duplicate of a keyword, for Shortest the FIRST).  "First" is first in the reference's
 * listener-call order -- for AhoCorasick end ascending, then start ascending, which is not the lowest start: keywords "abc" and
 * "b" on "abc" give "b".
 *  out       : HOST array of n_haystacks entries, overwritten; a size that does not depend on the matches, so there is no capacity
 *              to guess and never ACGPU_E_OVERFLOW.
 *  st        : NULL, or n_records = the sum of n_matches, n_matched = the haystacks with n_matches > 0; pieces and rescans are those
 *              of the one text the haystacks are scanned as (of the texts per haystack, summed, where the library scans those).
 *  errors    : ACGPU_E_INVALID, before any device is touched: NULL a or offsets; NULL out with n_haystacks > 0; descending offsets;
 *              units to read and no array; offsets[n_haystacks] - offsets[0] + n_haystacks >= 2^31.  ACGPU_E_INVALID as well with
 *              tickets in flight on the pool (the call works on the NULL stream, under the pool's lock, as the batch match call).
 *              n_haystacks == 0: ACGPU_OK, nothing but *st is written, no device needed.  Without a device the call fails as
 *              acgpu_match_batch_u16 does.  After every failure `out` is untouched.
 * How it works: the haystacks are concatenated with a separator unit behind each, as acgpu_match_batch_u16 does, and that text
 * goes through the pieces of a counting call (the same ramp and rescan rules; the Map records of a piece stay in the pool's
 * reservoir).  Behind every piece that completed, k_batch_summary runs over its records, a lane per record: a haystack's records
 * are contiguous in every family's order, so the piece's list is a sequence of runs, one per haystack; the head of a run adds
 * minus its index to the haystack's count and the tail its index plus one -- two 64-bit atomics per run and piece, whatever its
 * length, and a run that a piece boundary cuts still sums to its length -- and a head writes its record as the first one where
 * none is written yet.  The summaries (24 bytes per haystack) are copied out once, at the end; per piece the host waits only for
 * what the scan itself waits for.
 * Haystack by haystack inside the library instead, same results, where acgpu_match_batch_u16 falls back (a dictionary that uses
 * all 65536 units, and the word matchers over a table that is not fold-consistent): every haystack goes through the pieces as a
 * text of its own, into its own entry; no host buffer grows with the matches there either.
 * Not built: a device-resident, multi-device or streaming form of this call; stopping a haystack's scan at its first match (the
 * scan still finds every record: what is saved is their way to the host); the Java facade.  ACGPU_ABI_VERSION stays as it is:
 * adding symbols is compatible.
 */
typedef struct acgpu_batch_summary {
    uint64_t n_matches;              /* records acgpu_match_batch_u16 (ACGPU_REC_MAP) returns for this haystack          */
    int32_t start, end, keyword_id;  /* the FIRST of them in the reference's listener-call order, positions relative to
                                        the haystack, id as in a Map record; -1, -1, -1 when n_matches == 0             */
    int32_t reserved;                /* 0 */
} acgpu_batch_summary;               /* 24 bytes */
typedef struct acgpu_summary_stats {
    uint64_t n_records;       /* sum of n_matches                                  */
    uint64_t n_matched;       /* haystacks with n_matches > 0                      */
    uint32_t pieces, rescans; /* as acgpu_replace_stats                            */
} acgpu_summary_stats;
int acgpu_summary_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                            acgpu_batch_summary *out /* n_haystacks, host */, acgpu_summary_stats *st /* may be NULL */);

/*
 * A haystack in UTF-8 -- text as it lies in a file or in a buffer of a C, Python, Go or Rust caller -- in HOST memory: validated
 * and transcoded to UTF-16 on the device, scanned there, and the records returned in BYTE offsets of `bytes`.  The call returns
 * the records acgpu_match_u16 returns for the decoded text (what bytes.decode("utf-8") followed by a Java String of it holds):
 * their number, order, keyword_id and record_kind are the same, every family; only start and end differ, `end` exclusive.
 * MAPPING RULE.  start becomes the offset of the first byte of the encoded code point that holds unit `start`; end becomes one
 * past the last byte of the code point that holds unit `end - 1`.  For a match on code-point boundaries that is the obvious
 * mapping.  A match that begins or ends between the two units of a surrogate pair -- possible only with keywords that hold
 * lone surrogates -- gets the smallest byte span that covers it: all four bytes of that code point are inside.
 * VALIDATION is strict, as in CPython's bytes.decode("utf-8"): stray or missing continuation bytes, a sequence truncated by the
 * end of the text, overlong forms (leads C0 / C1, E0 80..9F, F0 80..8F), encoded surrogates (ED A0..BF) and anything above
 * U+10FFFF (F4 90.., leads F5..FF) are ill-formed.  Then the call returns ACGPU_E_ENCODING, *n_out = 0, nothing has been scanned,
 * and stats->first_bad is the smallest offset that is the lead byte of an ill-formed sequence or a continuation byte that no
 * lead claims -- the value of CPython's UnicodeDecodeError.start.  A byte order mark is not stripped: U+FEFF is a unit like any
 * other.
 *  n_bytes   : < 2^31, else ACGPU_E_INVALID (as NULL a, bytes or n_out, and a bad record_kind: before a device is touched).
 *              n_bytes == 0: ACGPU_OK, no records, no device needed.
 *  out, cap, *n_out : as for acgpu_match_u16; on ACGPU_E_OVERFLOW *n_out is the capacity to retry with (cap 0 and out NULL: count).
 *  stats     : NULL, or what the transcoder found.  ascii == 1: every byte is below 0x80, unit offsets ARE byte offsets and the
 *              records were not rewritten.
 * Works on the NULL stream, under the pool's lock (STREAM RULE above: tickets in flight on the pool give ACGPU_E_INVALID).
 * How it works: the bytes are copied to the device; k_utf8_count validates them, a lane per 16 bytes, and counts the units of
 * every block of 4096 bytes; the host waits ONCE for 16 bytes (n_units, first_bad) to size the shard; k_utf8_write stores the
 * units and, per 32 units, the byte offset of the sequence that holds the first of them (the checkpoints); the scan is
 * match_shard on the whole text as one shard, unchanged; k_utf8_batch_map rewrites start and end - 1 of every record in place from
 * the nearest checkpoint and a walk of at most 31 units over the lead bytes; one copy brings the records out.
 * The call is ONE shard through the general path: neither the chunk-pipelined form acgpu_match_u16 takes from 2^25 units on
 * (a long text is copied whole before the scan begins, nothing overlaps), nor its one-launch form for texts of up to 4096 units
 * (a short text pays the fixed cost of five launches, two copies and two waits, several times that form's latency: batch short
 * texts with acgpu_match_batch_utf8 / acgpu_summary_batch_utf8 below).  A text that arrives in chunks, or is longer than 2^31
 * bytes: acgpu_stream_feed_utf8 below.  Not built: count, cursor, the pipelined stream,
 * device-resident and multi-device forms for UTF-8 (replace: acgpu_replace_utf8 and acgpu_replace_batch_utf8 below; lossy decoding,
 * ill-formed bytes scanned as U+FFFD: acgpu_match_utf8_lossy below); CESU-8 / WTF-8;
 * the Java facade (its strings are UTF-16).  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
typedef struct acgpu_utf8_stats {
    uint64_t n_units;    /* UTF-16 units the text decodes to (0 on ACGPU_E_ENCODING)                */
    int64_t  first_bad;  /* -1, or the byte offset of the first ill-formed sequence                 */
    uint32_t ascii;      /* 1: every byte < 0x80, offsets were not remapped                         */
    uint32_t reserved;
} acgpu_utf8_stats;
int acgpu_match_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap,
                     uint64_t *n_out, acgpu_utf8_stats *stats /* may be NULL */);

/*
 * Replace for a UTF-8 text in HOST memory: bytes in, rewritten bytes out, nothing decoded or encoded on the host.  With
 * r_0 .. r_{k-1} the Map records acgpu_match_utf8 returns for `bytes` (BYTE offsets), in their order, the result is
 *   bytes[0:s_0] + repl[id_0] + bytes[e_0:s_1] + repl[id_1] + ... + bytes[e_{k-1}:n_bytes]
 * -- outside the matches a byte-for-byte copy of the caller's buffer; nothing is re-encoded.
 *  repl_bytes / repl_off / n_repl : the table of acgpu_replace_u16 with BYTES for units: replacement i is
 *              repl_bytes[repl_off[i] .. repl_off[i+1]), n_repl is the number of keywords given to acgpu_build or 1, an empty
 *              entry deletes the match.  The bytes are copied as given and NOT validated: the result is well-formed UTF-8 when
 *              every replacement is.
 *  cap, *n_out : in BYTES, as for acgpu_replace_u16: a result of more than cap bytes gives ACGPU_E_OVERFLOW with *n_out (and
 *              st->units_out, which counts bytes here) exact, nothing at or beyond out[cap] written; out == NULL with cap == 0
 *              counts only.
 *  families  : ACGPU_MODE_LONGEST, _SHORTEST, _WHOLEWORD, _WWLONGEST.  ACGPU_MODE_ALL: ACGPU_E_UNSUPPORTED.  An automaton one of
 *              whose keywords holds an UNPAIRED SURROGATE: ACGPU_E_UNSUPPORTED as well -- by the mapping rule a match that begins
 *              or ends inside a surrogate pair covers all four bytes of the code point, so two records could cover the same
 *              bytes, and replace rests on records that do not overlap.  With well-formed keywords every record begins and ends
 *              on a code-point boundary, and records that do not overlap in units do not overlap in bytes.  Both refusals come
 *              before any device is touched, as do the ACGPU_E_INVALID of NULL a, bytes or n_out, cap without out,
 *              n_bytes >= 2^31 and a bad replacement table.
 *  ill-formed input : ACGPU_E_ENCODING with ust->first_bad as for acgpu_match_utf8; *n_out = 0, `out` is untouched, the pool
 *              stays usable.
 *  n_bytes == 0 : ACGPU_OK, *n_out = 0, no device needed.
 *  st, ust   : may be NULL.  st->n_records: matches replaced; st->units_out: bytes of the result; ust as acgpu_match_utf8 fills it.
 * Works on the NULL stream, under the pool's lock (STREAM RULE above: tickets in flight on the pool give ACGPU_E_INVALID).
 * How it works: the text is staged as acgpu_match_utf8 stages it (validated, transcoded, checkpoints) and scanned in UNITS
 * through the pieces of acgpu_replace_device; behind every piece k_utf8_batch_map rewrites its records in the reservoir to byte
 * offsets, and one lane maps the piece's boundary to the first byte of the code point that holds it (rounded down: that only
 * withholds more).  From there on everything counts bytes: the plan runs unchanged over byte records and a byte table, and the
 * byte form of the emit kernel writes 16 output bytes per lane from the caller's bytes on the device and the table, through
 * the two slabs of acgpu_replace_u16 ("replace_slab_units" counts bytes here).
 * Many short texts in one call: acgpu_replace_batch_utf8 below.  One long text in chunks: acgpu_stream_replace_utf8 below.
 * Not built: device-resident and multi-device forms; validating the replacements; the Java facade.
 * ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
int acgpu_replace_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const uint8_t *repl_bytes,
                       const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                       acgpu_replace_stats *st /* may be NULL */, acgpu_utf8_stats *ust /* may be NULL */);

/*
 * Batches of UTF-8 haystacks in HOST memory: acgpu_match_batch_u16 and acgpu_summary_batch_u16 for texts as they lie in files --
 * log lines, JSON records, form fields -- in ONE device call.  Haystack i is bytes[offsets[i] .. offsets[i+1]) (the offsets
 * convention of acgpu_match_batch_u16: n_haystacks + 1 ascending offsets, empty haystacks allowed anywhere); the haystacks are
 * contiguous in the caller's buffer, which is copied to the device as it lies, once.
 *  acgpu_match_batch_utf8 returns the records acgpu_match_batch_u16 returns for the haystacks decoded one by one --
 *              acgpu_batch_set_match / acgpu_batch_map_match, the same count, order, haystack index and keyword_id, every
 *              family -- with start and end as BYTE offsets relative to the haystack's first byte, by acgpu_match_utf8's MAPPING
 *              RULE (the case inside a surrogate pair included).  On ACGPU_E_OVERFLOW *n_out is the capacity to retry with.
 *  acgpu_summary_batch_utf8 returns out[i] = {count, first record} of those records for haystack i, the first record in byte
 *              offsets relative to the haystack; all five families; never ACGPU_E_OVERFLOW.  st as acgpu_summary_batch_u16 fills it.
 * VALIDATION is strict and PER HAYSTACK: every haystack must be well-formed on its own, as
 * bytes[offsets[i]:offsets[i+1]].decode("utf-8") in CPython.  A sequence that a haystack boundary cuts is ill-formed, also where
 * the next haystack's first bytes would complete it: "a\xc3" | "\xa9b" is refused at haystack 0, offset 1, although the buffer
 * as a whole is valid.  Then the call returns ACGPU_E_ENCODING; stats->bad_haystack is the first ill-formed haystack and
 * stats->first_bad the offset inside it at which a strict decoder stops (UnicodeDecodeError.start of that haystack); *n_out = 0,
 * `out` is untouched, nothing has been scanned, the stream is idle and the pool is usable.
 * ACGPU_E_INVALID, before a device is touched and with out and stats untouched: NULL a, offsets or n_out, cap without out (the
 * summary: haystacks without out), a bad record_kind, descending offsets, bytes NULL with a byte to read, and
 * offsets[n] - offsets[0] + n_haystacks >= 2^31 (bytes >= units, so this bounds the text the scan sees as well).
 * n_haystacks == 0, or all haystacks empty: ACGPU_OK without a device; the summary fills {0, -1, -1, -1, 0}.
 * Both work on the NULL stream, under the pool's lock (STREAM RULE above: tickets in flight on the pool give ACGPU_E_INVALID).
 * How it works: k_utf8_batch_count is k_utf8_count with a twelfth mask, `cut`, a bit where a byte begins a haystack: a lead is
 * bad when a byte it needs lies at or behind a cut, a continuation byte at a cut is unclaimed; the smallest flagged offset of the
 * buffer is then the first ill-formed haystack's own error position, and the host turns it into (bad_haystack, first_bad).
 * k_utf8_batch_write stores the units with the builder's separator unit behind every haystack -- the text acgpu_match_batch_u16
 * scans -- and every haystack's first unit in it; the checkpoints stay indexed by the unit WITHOUT separators.  The scan is
 * match_shard on that one shard (the summary: the pieces of acgpu_summary_batch_u16 over it, k_batch_summary behind each);
 * k_utf8_batch_tag, a lane per record, finds the haystack and maps start and end - 1 to bytes relative to it
 * (k_summary_utf8_bytes, a lane per haystack, the summaries' first records).  An all-ASCII batch writes no checkpoints and maps
 * nothing.  Where acgpu_match_batch_u16 goes haystack by haystack (no free separator unit, a word matcher over a table that is
 * not fold-consistent) these do too, after the same validation of the whole batch: one acgpu_match_utf8-style pass per haystack.
 * Batch replace: acgpu_replace_batch_utf8 below.  One long text in chunks: acgpu_stream_feed_utf8 below.  Not built:
 * acgpu_count_utf8; device-resident, multi-device and cursor forms; the one-launch form for tiny batches; the Java facade.  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
typedef struct acgpu_utf8_batch_stats {
    uint64_t n_units;      /* UTF-16 units of all haystacks, separators not counted (0 on ACGPU_E_ENCODING) */
    int64_t  first_bad;    /* -1, or the offset INSIDE haystack bad_haystack at which a strict decoder stops */
    uint32_t bad_haystack; /* the first haystack that is ill-formed (0 when first_bad == -1)                 */
    uint32_t ascii;        /* 1: every byte < 0x80                                                           */
} acgpu_utf8_batch_stats;  /* 24 bytes */
int acgpu_match_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks, int record_kind,
                           void *out, uint64_t cap, uint64_t *n_out, acgpu_utf8_batch_stats *stats /* may be NULL */);
int acgpu_summary_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                             acgpu_batch_summary *out /* n_haystacks, host */, acgpu_summary_stats *st /* may be NULL */,
                             acgpu_utf8_batch_stats *stats /* may be NULL */);

/*
 * LOSSY UTF-8: acgpu_match_utf8, acgpu_match_batch_utf8 and acgpu_summary_batch_utf8 for bytes that need not be well-formed -- log
 * files, crash dumps, scraped text, truncated lines.  Nothing is refused: the call returns the records its strict counterpart
 * would return for bytes.decode("utf-8", errors="replace") of the text (a batch: of every haystack on its own) -- the same count,
 * order and keyword_id, every family -- with start and end as BYTE offsets of the caller's own, unmodified buffer.
 * REPLACEMENT is CPython's: every MAXIMAL ILL-FORMED SUBPART becomes ONE U+FFFD.  A subpart is one to three bytes: a lead byte
 * with the longest run of following bytes that is still a valid prefix for that lead (the second byte in the range the lead
 * allows -- E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F -- the others continuation bytes), or a single byte that can begin
 * nothing: a continuation byte that no lead claims, C0, C1, F5..FF.  So E0 80 80 is three U+FFFD, F0 9F 28 is one (two bytes)
 * and "(", F0 9F 98 at the end of the text is one of three bytes.
 * MAPPING RULE.  A U+FFFD that stands for a subpart maps to that subpart's bytes: start is its first byte, end one past its
 * last.  Everything else follows acgpu_match_utf8's MAPPING RULE.  A keyword that holds U+FFFD matches a genuine EF BF BD and a
 * replaced subpart alike, as on the decoded string.
 * BATCH.  Haystack i is decoded alone, as bytes[offsets[i]:offsets[i+1]].decode("utf-8", "replace"): a sequence that a haystack
 * boundary cuts is a subpart that ends at the boundary, and the continuation bytes at the begin of the next haystack are one
 * U+FFFD each -- "a\xc3" | "\xa9b" is a, U+FFFD | U+FFFD, b.
 * Everything else is the strict counterpart's, whose body these share: ACGPU_E_INVALID before a device is touched, the empty text
 * and the all-empty batch without a device, ACGPU_E_OVERFLOW, the NULL stream under the pool's lock, and the haystack-by-haystack
 * route where acgpu_match_batch_utf8 takes it.  ACGPU_E_ENCODING is never returned.
 *  stats     : NULL, or what the decoder found.  ascii == 1: every byte is below 0x80.  A text with as many units as bytes
 *              ("a\x80b": every start one byte and one unit) is mapped by the identity as an ASCII text is, but ascii is 0 as soon
 *              as anything was replaced.
 * How it works: the LOSSY forms of the strict kernels.  The masks of a lane come from claimed_lossy -- a lead claims the byte
 * behind it only in the range it allows, the next ones only behind a claimed one, never a byte at or behind a haystack boundary --
 * so a start is every byte that is no claimed continuation byte, and a replaced start is a lead that did not claim all it needs or
 * an unclaimed continuation byte; on well-formed bytes every mask equals the strict one.  k_utf8_lossy_count adds the replaced
 * starts of a wave with one 64-bit atomic where there are any, the first of them goes through the strict kernels' atomicMin, and
 * the one wait brings n_replaced with n_units.  k_utf8_lossy_write stores 0xFFFD for a replaced start and, beside the checkpoints,
 * a START BITMAP: a bit per byte, set where a sequence or a subpart begins, 16 bits per lane in one store.  The maps walk that
 * bitmap from the checkpoint, not the bytes: a start's length is the distance to the next set bit, and it has two units exactly
 * when that is 4 (a subpart has at most 3 bytes).  The bitmap holds the haystack boundaries, so a walk that begins in an earlier
 * haystack needs to know nothing about them.
 * Replace, batch replace, the stream feed and stream replace in lossy form: acgpu_replace_utf8_lossy,
 * acgpu_replace_batch_utf8_lossy, acgpu_stream_feed_utf8_lossy and acgpu_stream_replace_utf8_lossy below.
 * Not built in lossy form: errors="ignore" (drop the bytes), the Java facade.  ACGPU_ABI_VERSION stays as it is: adding symbols
 * is compatible.
 */
typedef struct acgpu_utf8_lossy_stats {
    uint64_t n_units;         /* units the text decodes to, replacements included; batch: separators not counted */
    uint64_t n_replaced;      /* U+FFFD units that stand for ill-formed subparts (exact)                           */
    int64_t  first_replaced;  /* -1, or the byte offset of the first of them; batch: inside haystack first_haystack */
    uint32_t first_haystack;  /* batch: the haystack that holds it (0 otherwise)                                   */
    uint32_t ascii;           /* 1: every byte < 0x80 (then n_replaced == 0)                                       */
} acgpu_utf8_lossy_stats;     /* 32 bytes */
int acgpu_match_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int record_kind, void *out, uint64_t cap,
                           uint64_t *n_out, acgpu_utf8_lossy_stats *stats /* may be NULL */);
int acgpu_match_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                 int record_kind, void *out, uint64_t cap, uint64_t *n_out, acgpu_utf8_lossy_stats *stats /* may be NULL */);
int acgpu_summary_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                   acgpu_batch_summary *out /* n_haystacks, host */, acgpu_summary_stats *st /* may be NULL */,
                                   acgpu_utf8_lossy_stats *stats /* may be NULL */);

/*
 * Many short texts COUNTED PER KEYWORD in one call: the document-term matrix of a batch -- which keywords of the dictionary occur
 * in every haystack, and how often -- reduced on the device, in CSR form.  Row i holds the distinct keyword_ids of the records with
 * haystack == i that acgpu_match_batch_u16(..., ACGPU_REC_MAP, ...) returns for the same arguments, ascending, each with the
 * number of such records: numpy's unique(ids, return_counts=True) per haystack.  Every family, ACGPU_MODE_ALL included.  Ids
 * index the list given to acgpu_build, as in acgpu_count_u16: the matrix has as many columns as keywords were given, and a
 * duplicate keyword reports the index that wins in the match call.  No positions are returned, so the UTF-8 forms map nothing: they
 * return what acgpu_count_batch_u16 returns for the haystacks decoded one by one (the lossy form: decoded with errors="replace").
 * A single text is a batch of one haystack: that is also how a UTF-8 text gets sparse counts per keyword.
 *  row_ptr     : HOST, n_haystacks + 1 entries; row i is [row_ptr[i], row_ptr[i + 1]) of keyword_ids and counts; row_ptr[0] == 0.
 *  keyword_ids : HOST, cap entries (NULL allowed with cap == 0); ascending and distinct within a row.
 *  counts      : HOST, cap entries (NULL allowed with cap == 0).  32 bits suffice: one keyword ends at most once per unit, and a
 *                batch has fewer than 2^31 units.
 *  *n_out      : on success the stored entries, n_terms == row_ptr[n_haystacks].
 *  st          : NULL, or the call's numbers (written on success and on ACGPU_E_OVERFLOW).
 * CAPACITY.  The device produces ENTRIES {haystack, keyword, count}, and a haystack whose records are cut -- see below -- has
 * the same keyword in more than one of them until the host has merged them: n_terms <= n_entries <= n_records.  cap is compared
 * with n_entries.  If n_entries > cap the call returns ACGPU_E_OVERFLOW with *n_out = n_entries -- exact, counting goes on where
 * writes are dropped -- and nothing is written to the three arrays.  The same call again (the same automaton, batch and tunables)
 * with cap >= that *n_out succeeds: the pieces and blocks of a call depend on nothing else, so it produces the same entries.
 * cap = the batch's record count always suffices.
 *  errors    : ACGPU_E_INVALID, before any device is touched: NULL a, offsets, row_ptr or n_out; cap > 0 with NULL keyword_ids or
 *              counts; descending offsets; units to read and no array; offsets[n_haystacks] - offsets[0] + n_haystacks >= 2^31 (the
 *              UTF-8 forms: in bytes).  ACGPU_E_INVALID as well with tickets in flight on the pool (the call works on the NULL
 *              stream, under the pool's lock, as acgpu_summary_batch_u16 does).  ACGPU_E_ENCODING (acgpu_count_batch_utf8 only): as
 *              acgpu_summary_batch_utf8 reports it, stats->bad_haystack and stats->first_bad; *n_out = 0.  n_haystacks == 0, or all
 *              haystacks empty: ACGPU_OK with an empty matrix, no device needed.  Without a device the call fails as
 *              acgpu_match_batch_u16 does.  After every failure the three arrays are untouched.
 * How it works: the haystacks go through the pieces as acgpu_summary_batch_u16 drives them (one text with a separator unit behind
 * every haystack; the Map records of a piece stay in the pool's reservoir; a piece scanned again for want of room is reduced
 * once).  A family's records come in listener order and no match crosses a separator, so the haystack index of the records never
 * descends.  Behind every piece three kernels run, with no host wait: k_terms_block -- a workgroup of 256 lanes per block of 2048
 * consecutive records sorts the keys (haystack << 32) | id in LDS with a bitonic network, marks the heads of the runs of equal
 * keys, and writes its distinct {haystack, id, count} to its own region of a staging buffer; k_terms_place -- one workgroup scans
 * the blocks' numbers of distinct keys behind the call's running entry count; k_terms_gather -- every block copies its entries to
 * their place in the call's entry list, where that is below cap.  The list has the haystacks ascending, and within one block's
 * entries of one haystack the ids ascending and distinct.  A haystack whose run of records is CUT by a block boundary or a piece
 * boundary, or that has more than 2048 records, has several such sub-rows in a row.  At the end the list is copied to the host
 * once (12 bytes per entry) and finished in one linear pass: row_ptr is filled, and only the cut rows -- one per 2048 records
 * where haystacks are short -- are sorted and their equal ids summed (st->rows_cut).
 * THE LIMIT of this form: one huge haystack is one row cut into as many sub-rows as it has blocks, and the host then sorts all of
 * its entries on one thread; short texts are the contract of the batch calls.
 * Haystack by haystack inside the library instead, same results, where acgpu_match_batch_u16 falls back (a dictionary that uses
 * all 65536 units, and the word matchers over a table that is not fold-consistent): every haystack goes through the pieces as a
 * text of its own and the same kernels.
 * Memory, kept by the pool and grow-only: the entry list, 12 bytes per entry up to cap (it grows with the records seen, never past
 * cap); the staging buffer, 12 bytes per record of ONE piece rounded up to 2048 records, plus 12 bytes per block; the counting
 * calls' reservoir; and what acgpu_summary_batch_u16 (the UTF-8 forms: acgpu_summary_batch_utf8) needs without the summaries.
 * Not built: a dense per-keyword count of a UTF-8 text; device-resident, multi-device, cursor or streaming forms; a merge of the
 * cut rows on the device; document frequency and other reductions of the matrix; the Java facade.  ACGPU_ABI_VERSION stays as it
 * is: adding symbols is compatible.
 */
typedef struct acgpu_count_batch_stats {
    uint64_t n_records;       /* records of the batch: the sum of all counts                                    */
    uint64_t n_entries;       /* entries the device produced, before cut rows are merged: what cap is compared with */
    uint64_t n_terms;         /* entries of the matrix (0 on ACGPU_E_OVERFLOW)                                    */
    uint32_t pieces, rescans; /* as acgpu_summary_stats                                                           */
    uint32_t rows_cut;        /* rows the host had to sort and merge                                              */
    uint32_t reserved;        /* 0 */
} acgpu_count_batch_stats;    /* 40 bytes */
int acgpu_count_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                          uint64_t *row_ptr /* n_haystacks + 1, host */, uint32_t *keyword_ids /* cap, host */, uint32_t *counts /* cap, host */,
                          uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st /* may be NULL */);
int acgpu_count_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                           uint64_t *row_ptr /* n_haystacks + 1, host */, uint32_t *keyword_ids /* cap, host */, uint32_t *counts /* cap, host */,
                           uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st /* may be NULL */,
                           acgpu_utf8_batch_stats *stats /* may be NULL */);
int acgpu_count_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                 uint64_t *row_ptr /* n_haystacks + 1, host */, uint32_t *keyword_ids /* cap, host */,
                                 uint32_t *counts /* cap, host */, uint64_t cap, uint64_t *n_out, acgpu_count_batch_stats *st /* may be NULL */,
                                 acgpu_utf8_lossy_stats *stats /* may be NULL */);

/*
 * Many short UTF-8 texts rewritten in ONE call: acgpu_replace_utf8 for a batch, the conjunction of acgpu_match_batch_utf8 and
 * acgpu_replace_batch_u16.  Haystack i is bytes[offsets[i] .. offsets[i+1]) as for acgpu_match_batch_utf8 (contiguous in the
 * caller's buffer, empty ones allowed anywhere), and out[out_offsets[i] .. out_offsets[i+1]) is byte for byte what
 * acgpu_replace_utf8 returns for haystack i alone.  The results lie back to back; out_offsets has n_haystacks + 1 entries,
 * out_offsets[0] == 0 and *n_out == out_offsets[n_haystacks].
 *  repl_bytes / repl_off / n_repl, cap, *n_out, st : in BYTES, as for acgpu_replace_utf8; the replacements are not validated.
 *              st->n_records is the sum over the haystacks, st->units_out == *n_out.
 *  refusals  : before any device is touched.  The replacement table is checked first (ACGPU_E_INVALID; ACGPU_E_UNSUPPORTED for
 *              ACGPU_MODE_ALL), then ACGPU_E_UNSUPPORTED for a dictionary with an unpaired surrogate (see acgpu_replace_utf8), then
 *              ACGPU_E_INVALID for descending offsets, a byte to read and no `bytes`, and
 *              offsets[n_haystacks] - offsets[0] + n_haystacks >= 2^31.  NULL a, offsets, n_out or out_offsets and cap without out
 *              are ACGPU_E_INVALID before all of these.  After such a refusal out and out_offsets are untouched.
 *  no device : n_haystacks == 0, or every haystack empty: ACGPU_OK, *n_out = 0, every entry of out_offsets 0, *ust = {0, -1, 0, 1}.
 *  VALIDATION: strict and PER HAYSTACK, exactly as in acgpu_match_batch_utf8 -- a sequence that a haystack boundary cuts is
 *              ill-formed.  ACGPU_E_ENCODING with ust->bad_haystack / ust->first_bad; *n_out = 0, out and out_offsets[1..] are
 *              untouched, the stream is idle and the pool usable.
 *  overflow  : a result of more than cap bytes gives ACGPU_E_OVERFLOW; *n_out and EVERY entry of out_offsets are exact all the
 *              same (the plan runs to the end), and nothing at or beyond out[cap] has been written.  out == NULL with cap == 0
 *              only counts.
 * Works on the NULL stream, under the pool's lock (STREAM RULE above: tickets in flight on the pool give ACGPU_E_INVALID).
 * How it works: the batch is staged as acgpu_match_batch_utf8 stages it -- validated with the cuts, transcoded with a separator
 * unit behind every haystack -- and that shard goes through the pieces of acgpu_replace_utf8.  The caller's bytes have NO
 * separator, so, unlike acgpu_replace_batch_u16, nothing is merged and nothing deleted; three mappings take the scan's
 * coordinates to bytes of the span instead.  (1) Behind every piece k_utf8_batch_map rewrites its records in the reservoir: a
 * record of haystack h stands h separators behind its units in the checkpoint table, so units start - h and end - 1 - h go
 * through the checkpoints -- in an all-ASCII batch, which has none, the shift alone remains and is still applied.  (2) One lane,
 * k_utf8_batch_pos, maps the piece's boundary: a separator (the batch's last one included) to the byte where the next haystack
 * begins, any other unit to the first byte of the code point that holds it, rounded down.  (3) Behind the plan
 * k_replace_span_offsets, a lane per haystack boundary that the piece emits, computes where that haystack's result begins from
 * the plan's position of the last record in front of it; every boundary is written by exactly one piece, and the offsets leave
 * the device once, at the end.  Plan and the byte form of the emit run as they are.
 * Haystack by haystack inside the library instead, same results, where acgpu_match_batch_utf8 falls back (no free separator unit,
 * a word matcher over a table that is not fold-consistent): the whole batch is validated first, so what is refused does not
 * depend on the route, then every haystack takes acgpu_replace_utf8's route with cap, the output position and the stats carried
 * across and the table uploaded once.
 * Not built: device-resident, multi-device and cursor forms, a stream of batches (one long text in chunks:
 * acgpu_stream_replace_utf8 below); validating the replacements; a one-launch form for tiny batches; the Java facade.  Lossy form: acgpu_replace_batch_utf8_lossy below.  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
int acgpu_replace_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                             const uint8_t *repl_bytes, const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap,
                             uint64_t *out_offsets /* n_haystacks + 1 */, uint64_t *n_out,
                             acgpu_replace_stats *st /* may be NULL */, acgpu_utf8_batch_stats *ust /* may be NULL */);

/*
 * The chunked feed for UTF-8: match(Readable, ...) over a file, a dump or a socket as its BYTES arrive, records in byte offsets.
 * A stream opened with acgpu_stream_open is fed bytes instead of units; the concatenation of the records over all feeds is,
 * record for record, what acgpu_match_utf8 returns for the concatenation of all bytes fed -- count, order, keyword_id and
 * record kind, all five families (the Readable rule for word tables that are not fold-consistent, as acgpu_stream_feed) -- and
 * a feed returns the records that have become decidable, as acgpu_stream_feed does.
 *  out    : cap records of record_kind; start / end follow acgpu_match_utf8's MAPPING RULE (inside a surrogate pair included) as
 *           int32 relative to *base, a GLOBAL BYTE position (bytes since the first feed, int64: a stream may run past 2^31 bytes).
 *  CUT SEQUENCES.  A feed may end inside a sequence.  If its last 1..3 bytes are a proper prefix of a well-formed sequence --
 *           the lead is valid and every byte present satisfies the rule that names it: the second byte lies in the range its lead
 *           allows (E0 A0..BF, ED 80..9F, F0 90..BF, F4 80..8F), the third is a continuation byte -- they are held back
 *           (stats->held) and decoded with the next feed.  Anything else is ill-formed NOW.  With final != 0 nothing is held: a
 *           truncated sequence is ill-formed at its lead.  This is codecs.getincrementaldecoder("utf-8")().decode(chunk, final)
 *           of CPython: the same feed fails, at the same place.  That includes its one exception to the rule above: a feed that
 *           is not final and ENDS with the two bytes ED A0..BF (an encoded surrogate, cut) holds them too, although no third byte
 *           completes them; the next feed, or the final one, then reports the same offset, that of the ED.
 *  ACGPU_E_ENCODING : *n_out = 0, `out` is untouched, nothing of this feed was scanned; stats->first_bad is the GLOBAL offset (it
 *           may lie in an earlier feed's bytes: the lead of a held prefix that the new bytes fail to complete).  The stream is
 *           finished, only close is valid; the pool is as usable as before.
 *  ACGPU_E_OVERFLOW : nothing was consumed; *n_out is the capacity to call the SAME feed again with (cap == 0, out == NULL: count).
 *  ACGPU_E_INVALID, before a device is touched: NULL s, n_out or base; bytes NULL with a byte to read; cap without out; a bad
 *           record_kind; a finished or detached stream; carried bytes + n_bytes >= 2^31; a stream that has been fed through
 *           acgpu_stream_feed -- and acgpu_stream_feed on a stream that has been fed bytes.  The first feed of any kind, a feed
 *           of length 0 included, decides which of the four kinds the stream is (match units, match bytes, and the two replace
 *           kinds below); every other entry then returns ACGPU_E_INVALID.
 *  ACGPU_E_UNSUPPORTED : a stream switched to the pipelined form (acgpu_stream_set_pipelined, which in turn refuses a stream of bytes).
 *  no device : an empty feed that is not final, and an empty final feed on a stream that holds nothing: ACGPU_OK, no records.
 *  stats  : may be NULL.
 * Device and lifetime as for acgpu_stream_feed.  Works on the pool's call stream, under the pool's lock (STREAM RULE above:
 * tickets in flight on the pool give ACGPU_E_INVALID).
 * How it works: the stream carries BYTES on code-point boundaries -- the carried text and behind it the held prefix -- with the
 * units they decode to, and its positions in both measures.  A feed stages [carried bytes | chunk] as acgpu_match_utf8 stages a
 * text, through the OPEN form of the validator unless it is the last (k_utf8_open_count: a lead in the last three bytes whose
 * sequence reaches behind the buffer is judged by the bytes that are there; if they pass it is not counted and the host reads
 * {n_units, first_bad, tail} in the one wait; k_utf8_write runs over the n - tail bytes before it).  The shard is cut by the
 * plan of acgpu_stream_feed in units, scanned by match_shard, and k_utf8_batch_map rewrites the records to bytes of the buffer (an
 * all-ASCII buffer: nothing to map).  The byte at which the carry is cut for the next feed is found on the host, walking back
 * from the end of the decoded bytes over the lead bytes; it is a code-point boundary, so where the plan's unit is a low
 * surrogate one unit more is carried -- left context that is longer than needed changes no record.
 * Lossy decoding (U+FFFD): acgpu_stream_feed_utf8_lossy below.
 * Not built: the pipelined and reserved forms for bytes; cursor, count, device-resident and multi-device forms; the Java facade
 * (its Readable hands out UTF-16).  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
typedef struct acgpu_utf8_stream_stats {
    uint64_t n_units;    /* UTF-16 units the bytes newly decoded by this feed came to (0 on ACGPU_E_ENCODING)                      */
    int64_t  first_bad;  /* -1, or the GLOBAL byte offset (bytes since the first feed) at which a strict decoder stops             */
    uint32_t ascii;      /* 1: every byte of this feed's buffer (carry included) < 0x80, nothing was remapped                      */
    uint32_t held;       /* 0..3: bytes at the end of this feed that begin a sequence the next feed must complete                  */
} acgpu_utf8_stream_stats;   /* 24 bytes */
int acgpu_stream_feed_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, int record_kind,
                           void *out, uint64_t cap, uint64_t *n_out, int64_t *base,
                           acgpu_utf8_stream_stats *stats /* may be NULL */);

/*
 * Stream replace: acgpu_replace_u16 / acgpu_replace_utf8 for a text that arrives in chunks of any size and may be longer than
 * 2^31 elements -- a log file, a dump, a socket.  A stream opened with acgpu_stream_open is fed through ONE of these two entries;
 * the first feed of any kind, an empty one included, decides what the stream is, and every other entry then returns
 * ACGPU_E_INVALID.  "Element" below: a UTF-16 unit for acgpu_stream_replace_u16, a byte for acgpu_stream_replace_utf8.
 *  result : let T be the concatenation of everything fed and r_0 .. r_{k-1} the Map records that acgpu_stream_feed /
 *           acgpu_stream_feed_utf8 deliver for T over all feeds.  The concatenation of out[0 .. *n_out) over all feeds is
 *             T[0:s_0] + repl[id_0] + T[e_0:s_1] + ... + T[e_{k-1}:]
 *           whatever the chunking.  For a fold-consistent word table that is element for element what acgpu_replace_u16 /
 *           acgpu_replace_utf8 return for T; over a word table that is not fold-consistent the STREAM's records are meant (the
 *           Readable loops, which fold in every lookup), not those of the String loop.
 *  a feed : delivers the rewrite of T[done_before : done_after).  done_after is the position before which no later record can
 *           start, by the rule of the replace pieces applied to the feed's owned range (what acgpu_stream_feed would decide now):
 *           LONGEST, WHOLEWORD, WWLONGEST: max(end of the owned range, end of the feed's last record); SHORTEST: max(last
 *           record's end, done_before, end of the owned range - (max_keyword_len - 1)); final != 0: the end of the text -- for
 *           bytes the end of the decoded bytes: a held prefix (acgpu_stream_feed_utf8, CUT SEQUENCES) is never delivered before
 *           the bytes that complete it.  So without matches a feed that is not final withholds at most max_keyword_len + 1 units
 *           (in bytes: at most 4 * (max_keyword_len + 2) + 3), a match that begins in the owned range is delivered whole, by that
 *           feed, however many chunks it took to arrive, and final flushes everything.
 *  repl_* / n_repl : the table of acgpu_replace_u16 / acgpu_replace_utf8.  The table of the feed that delivers a record applies;
 *           pass the same one every time.
 *  cap, *n_out : in elements.  ACGPU_E_OVERFLOW: nothing was committed, *n_out (and st->units_out) is the exact size of THIS
 *           feed's output, out[0 .. cap) is unspecified and nothing at or beyond cap has been written; call the SAME feed again.
 *  st     : may be NULL; this feed alone, st->units_out == *n_out.  ust (bytes): may be NULL, as acgpu_stream_feed_utf8 fills it.
 *  ACGPU_E_UNSUPPORTED, before any device is touched: ACGPU_MODE_ALL; a pipelined stream; for bytes a dictionary with an unpaired
 *           surrogate (see acgpu_replace_utf8).
 *  ACGPU_E_INVALID, before any device is touched and with out, st and ust untouched: NULL s or n_out, data without a buffer, cap
 *           without out, a finished or detached stream, a stream of another kind, a bad replacement table, n >= 2^31 or carried
 *           + n >= 2^31.  Tickets in flight on the pool: ACGPU_E_INVALID as well (STREAM RULE above).
 *  ACGPU_E_ENCODING (bytes): as acgpu_stream_feed_utf8 -- ust->first_bad is the GLOBAL offset, *n_out = 0, `out` is untouched,
 *           the stream is finished and the pool usable.  What earlier feeds had withheld is NOT delivered: the output so far ends
 *           where the last successful feed ended.
 *  no device : an empty feed that is not final, and an empty final feed on a stream that holds nothing: ACGPU_OK, *n_out = 0.
 * Device and lifetime as for acgpu_stream_feed.  Nothing of the stream lives on the device between two feeds (the table is
 * uploaded per feed), so any other call on the automaton -- other streams and replace calls with other tables included -- may
 * run between them.
 * How it works: no kernel of its own.  A feed builds [carry | chunk] as the match feeds do, cuts it by their plan, and drives the
 * pieces of the replace entries over the owned range (the reservoir, the ramp and the rescans; plan and emit; the slabs), scanned
 * by the Readable rule; `done`, 64 bits and global, travels from feed to feed on the host.  The carry always reaches back to
 * `done` (keep_from <= owned end - left context <= done); a feed that finds otherwise returns ACGPU_E_HIP.
 * Not built: pipelined and reserved forms, ACGPU_MODE_ALL, device-resident and multi-device forms, the Java facade.
 * ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
int acgpu_stream_replace_u16(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, const uint16_t *repl_units,
                             const uint64_t *repl_off, uint32_t n_repl, uint16_t *out, uint64_t cap, uint64_t *n_out,
                             acgpu_replace_stats *st /* may be NULL */);
int acgpu_stream_replace_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const uint8_t *repl_bytes,
                              const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                              acgpu_utf8_stream_stats *ust /* may be NULL */, acgpu_replace_stats *st /* may be NULL */);

/*
 * LOSSY replace and LOSSY streams: acgpu_replace_utf8, acgpu_replace_batch_utf8, acgpu_stream_feed_utf8 and acgpu_stream_replace_utf8
 * for bytes that need not be well-formed.  Nothing is refused and ACGPU_E_ENCODING is never returned; the decoding is that of the
 * lossy match entries above (every MAXIMAL ILL-FORMED SUBPART is one U+FFFD, and maps to the subpart's bytes).
 *
 * acgpu_replace_utf8_lossy, acgpu_replace_batch_utf8_lossy.  RESULT RULE: let r_0 .. r_{k-1} be the Map records that
 * acgpu_match_utf8_lossy returns for the buffer (a batch: those of acgpu_match_batch_utf8_lossy, haystack by haystack), in BYTE
 * offsets.  The result is
 *   T[0:s_0] + repl[id_0] + T[e_0:s_1] + ... + T[e_{k-1}:]
 * over the CALLER'S bytes T.  Outside the matches it is a byte-for-byte copy of the input, ILL-FORMED BYTES INCLUDED: nothing is
 * normalised to EF BF BD, and no byte the dictionary did not name is altered -- the rule of every replace entry here.  A keyword
 * that holds U+FFFD matches a replaced subpart (and a genuine EF BF BD); the subpart's bytes are then what is removed.  On
 * well-formed input the result is byte for byte that of the strict entry.  The result is well-formed UTF-8 only where the input
 * outside the matches and the replacements are.
 * Everything else is the strict counterpart's, whose body these share: the four families (ACGPU_MODE_ALL and a dictionary with an
 * unpaired surrogate: ACGPU_E_UNSUPPORTED), every ACGPU_E_INVALID before a device is touched and in the same order, the empty
 * text and the all-empty batch without a device, the overflow contract (exact *n_out and out_offsets, nothing at or beyond
 * out[cap] written), the NULL stream under the pool's lock, and the haystack-by-haystack route of the batch form.  ust: as
 * acgpu_match_utf8_lossy / acgpu_match_batch_utf8_lossy fill it (a batch: first_haystack and first_replaced inside it); preset
 * {0, 0, -1, 0, 1} where no device is needed.
 * How it works: the text is staged with the lossy kernels, the pieces scan its units, k_utf8_batch_map and k_utf8_batch_pos walk
 * the start bitmap for a piece's records and its boundary (rounded down to the first byte of the START that holds it: a subpart
 * is one unit, so only a surrogate pair rounds), and plan and emit run unchanged over the caller's bytes on the device.  No
 * kernel of their own but the lossy form of k_utf8_batch_pos.
 *
 * acgpu_stream_feed_utf8_lossy.  The records of all feeds together are those of acgpu_match_utf8_lossy on the concatenation of
 * everything fed, in GLOBAL byte offsets (start / end relative to *base), all five families, whatever the chunking.  Arguments,
 * ACGPU_E_OVERFLOW, ACGPU_E_INVALID, ACGPU_E_UNSUPPORTED and the feeds that need no device: as acgpu_stream_feed_utf8.
 *  CUT SEQUENCES, lossy.  A feed that is not final holds back its last 1..3 bytes exactly when they are a lead together with
 *           everything it has claimed so far (the second byte in the range its lead allows, later ones continuation bytes) AND
 *           that claim reaches the buffer's end while the lead still needs more.  Anything else is decided now: a lead whose
 *           present bytes already fail is a subpart now.  So ED A0 at the end of a feed is two U+FFFD at once -- the strict
 *           feed's exception, taken from CPython's incremental decoder, is not mirrored; what is promised is that the chunking
 *           changes nothing.  With final != 0 nothing is held: a held prefix becomes ONE U+FFFD of 1..3 bytes, as
 *           bytes.decode("utf-8", "replace") gives for a truncated tail.
 *  STREAM KIND.  The error policy is part of the stream's kind, fixed by its first byte feed (an empty one included): a strict
 *           byte feed on a lossy stream returns ACGPU_E_INVALID before any device is touched, and so does the reverse, for the
 *           match feeds and the replace feeds alike -- six kinds in all.
 *  stats  : may be NULL.  Summed over the feeds, n_units and n_replaced are those of acgpu_match_utf8_lossy on the whole text (the
 *           stream keeps the replaced count of the bytes it carries, so none is reported twice).
 * How it works: k_utf8_lossy_open_count, the validator that is both LOSSY and OPEN -- the held lead is neither a start nor
 * replaced, the bytes before it decode as a closed text exactly as they do open, so k_utf8_lossy_write runs unchanged over them.
 * One wait brings four words: res[0] n_units, res[1] the first replaced offset, res[2] the held bytes, res[3] n_replaced.  The
 * carry is cut at a START -- a lead, or a continuation byte nobody claimed -- which the host finds by restating the claim rule
 * over the few bytes it walks back from the end; the claim rule looks at most 3 bytes back.
 *
 * acgpu_stream_replace_utf8_lossy.  acgpu_stream_replace_utf8 over the lossy feed: the RESULT RULE above applied to the whole
 * stream, with the records of acgpu_stream_feed_utf8_lossy, and the strict entry's rule for what a feed delivers and withholds; a
 * held prefix is never delivered before the bytes that complete it (or fail to) or the final feed.  No kernel of its own.
 * Not built: errors="ignore"; normalising unmatched ill-formed bytes to EF BF BD; pipelined or reserved byte streams; the Java
 * facade; ACGPU_MODE_ALL.  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
typedef struct acgpu_utf8_lossy_stream_stats {
    uint64_t n_units;     /* units newly decoded by this feed, replacements included */
    uint64_t n_replaced;  /* of those, U+FFFD that stand for ill-formed subparts     */
    uint32_t ascii;       /* as acgpu_utf8_stream_stats; 0 as soon as the buffer holds anything replaced */
    uint32_t held;        /* 0..3                                                    */
} acgpu_utf8_lossy_stream_stats;   /* 24 bytes */
int acgpu_replace_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const uint8_t *repl_bytes,
                             const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                             acgpu_replace_stats *st /* may be NULL */, acgpu_utf8_lossy_stats *ust /* may be NULL */);
int acgpu_replace_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                   const uint8_t *repl_bytes, const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap,
                                   uint64_t *out_offsets /* n_haystacks + 1 */, uint64_t *n_out,
                                   acgpu_replace_stats *st /* may be NULL */, acgpu_utf8_lossy_stats *ust /* may be NULL */);
int acgpu_stream_feed_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, int record_kind,
                                 void *out, uint64_t cap, uint64_t *n_out, int64_t *base,
                                 acgpu_utf8_lossy_stream_stats *stats /* may be NULL */);
int acgpu_stream_replace_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const uint8_t *repl_bytes,
                                    const uint64_t *repl_off, uint32_t n_repl, uint8_t *out, uint64_t cap, uint64_t *n_out,
                                    acgpu_utf8_lossy_stream_stats *ust /* may be NULL */, acgpu_replace_stats *st /* may be NULL */);

/*
 * Spans: which parts of a text are covered by a match -- the records of a text merged into covered runs on the device, for ALL
 * FIVE families (ACGPU_MODE_ALL included: the answer the replace entries refuse it).  With R the Set records acgpu_match_u16
 * returns for the same automaton and text, the SPANS are the maximal runs of consecutive positions p with s <= p < e for some
 * record {s, e} of R: ascending, each {start, end} as two int32 (the layout of ACGPU_REC_SET).  Overlapping, nested AND touching
 * records fall into one span -- [1,5) and [5,8) give [1,8) -- so two consecutive spans have at least one uncovered position
 * between them.  The records of the four non-overlapping families can touch, so their spans are not their records either.
 *  cap, *n_out : in SPANS.  More than cap spans: ACGPU_E_OVERFLOW with *n_out (and st->n_spans) the exact number; out[0 .. cap)
 *              then holds the first cap spans and nothing at or beyond cap has been written (the rest of the text is still
 *              scanned and merged, for the number).  The same call with cap = *n_out succeeds.
 *  st        : may be NULL.
 *  acgpu_spans_u16    : haystack in HOST memory, n_units < 2^31; `out` is host memory.  Without a device it fails as
 *              acgpu_match_u16 does and leaves `out` untouched.  Works on the NULL stream (STREAM RULE above), under the pool's lock.
 *  acgpu_spans_device : the shard must be a WHOLE text (own_begin == 0, own_end == n_units, text_begin == text_end == 1), else
 *              ACGPU_E_UNSUPPORTED: one shard of a sharded text would have to hand the spans it withholds to the rank behind it,
 *              which is not built.  d_out: device memory, 16-byte aligned, written directly (clipped at cap).  Everything is
 *              enqueued on `stream`; the call waits for it per piece -- for the piece's record count and for its span count --
 *              and once at the end.
 *  acgpu_spans_utf8 / acgpu_spans_utf8_lossy : the spans of the records acgpu_match_utf8 / acgpu_match_utf8_lossy returns, in BYTE
 *              offsets of the caller's buffer; n_bytes < 2^31; ust and ACGPU_E_ENCODING as for those entries.  An empty text:
 *              ACGPU_OK, *n_out = 0, no device needed.  Keywords that hold an unpaired surrogate are accepted (their widened
 *              records may overlap in bytes, which a merge does not mind).
 * How it works: the text is cut into pieces as a cursor's are (the same ramp and rescan rules); a piece's Set records go to the
 * pool's reservoir, and five small launches behind the piece merge them -- a suffix minimum of the starts finds where a span
 * begins, a prefix count gives the span its index, the first and the last interval of a span write its two words (no atomics,
 * the result is deterministic).  A piece delivers the spans that end before a position no later record starts at or before; the
 * others -- at most max_keyword_len / 2 + 2 of them -- wait on the device for the next piece (st->max_carry: the most that did).
 * Scratch, per automaton and device: the reservoir the counting and replace calls use, 12 bytes per 2048 records of a piece, the
 * carry, and for the host entries 8 bytes per span of a piece.  The host reads 16 bytes per piece.
 *  acgpu_spans_batch_u16 : many short texts in one call.  Haystack i is units[offsets[i] .. offsets[i + 1]) as for
 *              acgpu_match_batch_u16 (empty haystacks allowed, the same ACGPU_E_INVALID: NULL a, offsets or n_out, descending
 *              offsets, a concatenation of 2^31 units or more, a cap without a buffer; n_haystacks == 0: ACGPU_OK, *n_out = 0, no
 *              device).  The result is {haystack, start, end} triples of int32 -- the layout of acgpu_match_batch_u16's Set
 *              records -- ordered by haystack and ascending within it, start and end relative to the haystack: the triples of
 *              haystack i are exactly the spans acgpu_spans_u16 returns for it alone.  cap, *n_out, overflow: in spans, as above.
 *              The haystacks are scanned as one text with a separator unit behind each; no record holds a separator and a
 *              separator is never covered, so the spans of that text are the haystacks' spans, shifted -- two spans that meet
 *              at a seam stay two.  A piece's final spans are tagged and rebased in the pool and leave 12 bytes each; no wait
 *              is added.  Where there is no free separator unit, or a word matcher's table is not fold-consistent, every
 *              haystack is scanned as a text of its own under the one lock (st->pieces then counts them all).  Works on the
 *              NULL stream, tickets in flight are refused (STREAM RULE), as acgpu_replace_batch_u16.
 *  acgpu_spans_batch_utf8, acgpu_spans_batch_utf8_lossy : the same for haystacks of BYTES: haystack i is
 *              bytes[offsets[i] .. offsets[i + 1]) of one buffer, as for acgpu_match_batch_utf8 (offsets[0] need not be 0; bytes
 *              plus haystacks below 2^31).  start and end are bytes relative to the haystack, and the triples of haystack i are
 *              the rows acgpu_spans_utf8 (_lossy) returns for it alone; keywords with an unpaired surrogate are served.  A batch
 *              without a byte: ACGPU_OK, *n_out = 0, no device.  Strict: every haystack must be well-formed on its own (a
 *              sequence cut by a boundary is ill-formed); ACGPU_E_ENCODING comes plainly after the transcoder's one wait with
 *              ust->bad_haystack and first_bad as acgpu_match_batch_utf8 sets them, *n_out = 0, out untouched and the stream
 *              idle, whichever way the batch would have been scanned.  Lossy: never ACGPU_E_ENCODING, every haystack decoded
 *              on its own.  How: the batch is staged once and scanned in units with a separator behind every haystack; a
 *              piece's records become positions in the caller's bytes with one phantom element behind every haystack (byte of
 *              the buffer + index of the haystack) where they lie, and the merge runs over those -- no record covers a phantom,
 *              so two spans that meet at a seam stay two, also where a keyword with an unpaired surrogate widens them.
 * Not built (mask, highlight and redaction on top of spans: the cover entries below): a record-free form for ACGPU_MODE_ALL from the
 * state words of k_ac_states (the analogue of the counting calls' direct form); stream and multi-device forms; the Java
 * facade.  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
typedef struct acgpu_spans_stats {
    uint64_t n_records;       /* records merged == records the Set match call returns                        */
    uint64_t n_spans;         /* spans of the text (exact, also on ACGPU_E_OVERFLOW)                         */
    uint32_t pieces, rescans; /* as acgpu_count_stats                                                        */
    uint32_t max_carry;       /* the largest number of spans a piece withheld for the next one               */
    uint32_t reserved;
} acgpu_spans_stats;   /* 32 bytes */
int acgpu_spans_u16(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, int32_t *out, uint64_t cap, uint64_t *n_out,
                    acgpu_spans_stats *st);
int acgpu_spans_device(const acgpu_automaton *a, acgpu_shard *shard, int32_t *d_out, uint64_t cap, uint64_t *n_out, void *stream,
                       acgpu_spans_stats *st);
int acgpu_spans_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                          int32_t *out /* 3 words per span */, uint64_t cap, uint64_t *n_out, acgpu_spans_stats *st /* may be NULL */);
int acgpu_spans_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                           int32_t *out /* 3 words per span */, uint64_t cap, uint64_t *n_out, acgpu_spans_stats *st /* may be NULL */,
                           acgpu_utf8_batch_stats *ust /* may be NULL */);
int acgpu_spans_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                 int32_t *out /* 3 words per span */, uint64_t cap, uint64_t *n_out, acgpu_spans_stats *st /* may be NULL */,
                                 acgpu_utf8_lossy_stats *ust /* may be NULL */);
int acgpu_spans_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int32_t *out, uint64_t cap, uint64_t *n_out,
                     acgpu_spans_stats *st, acgpu_utf8_stats *ust /* may be NULL */);
int acgpu_spans_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, int32_t *out, uint64_t cap, uint64_t *n_out,
                           acgpu_spans_stats *st, acgpu_utf8_lossy_stats *ust /* may be NULL */);

/*
 * Cover: mask, highlight or redact every covered run of a text, on the device, for ALL FIVE families.  Every span [s, e) of the
 * text -- exactly the spans the spans entries above report for the same automaton and text -- becomes open ++ body ++ close, and
 * everything outside the spans is copied as it is.  body is one of
 *   ACGPU_COVER_KEEP : the covered text itself (highlight, tagging: open = "<b>", close = "</b>")
 *   ACGPU_COVER_FILL : `fill` once per covered element, so with empty open and close the length is preserved (mask)
 *   ACGPU_COVER_DROP : nothing (open = "***": redaction; everything empty: deletion)
 * ELEMENTS are what the caller's text is made of: UTF-16 units for acgpu_cover_u16 and acgpu_cover_device, bytes for the UTF-8
 * entries (whose spans are in bytes, and which serve keywords with an unpaired surrogate as the spans entries do).  open and close
 * are HOST pointers in elements, uploaded once per call; the byte entries take them as they are, without validating them.
 *  not replace : overlapping, nested and TOUCHING records are one span, so DROP with open = r is the result of the replace entries
 *              with the single replacement r only where no two matches touch: two touching matches give one r, not two.
 *  fill      : a unit (<= 0xFFFF) in the unit entries, so a surrogate pair becomes two.  In the byte entries it must be below 0x80
 *              and is written once per covered BYTE: the result stays well-formed and every byte offset computed on the input
 *              holds on the output.  Lossy input: stray bytes inside a span are filled, outside the spans the output is a
 *              byte-for-byte copy, stray bytes included.  (fill is only looked at with ACGPU_COVER_FILL.)
 *  cap, *n_out : in ELEMENTS, as for the replace entries: a result of more than cap elements gives ACGPU_E_OVERFLOW with *n_out (and
 *              st->units_out) the exact size -- the text is scanned and planned to its end, out[0 .. cap) holds the result's
 *              first cap elements, nothing at or beyond cap has been written.  The same call with cap = *n_out succeeds.
 *  errors    : ACGPU_E_INVALID, before a device is touched: NULL a, spec or n_out; body > 2; a NULL pointer with a non-zero length
 *              (the text, out with cap, open, close); 2^31 or more elements of text, open or close; a fill that the entry's
 *              element does not hold (see above); acgpu_cover_device: d_hay not 16-byte aligned, d_out not aligned to a unit.
 *              ACGPU_E_UNSUPPORTED: a shard that is not a WHOLE text, as for acgpu_spans_device.  Ill-formed UTF-8, ust, the empty
 *              UTF-8 text (ACGPU_OK, *n_out = 0, no device) and the STREAM RULE: as for the spans entries.
 *  acgpu_cover_u16 : text and out in HOST memory.  The whole text is copied to the device in front of the first piece (one blocking
 *              copy): a span can reach across every piece, and KEEP copies its body long after the piece that first saw it.
 *  acgpu_cover_device : d_out is device memory of cap units at ANY unit address, written directly.
 * How it works: behind every piece the spans merge runs as for the spans entries, its final spans stay on the device, and with
 * their number the host reads the position up to which the text is settled -- in the one wait per piece that the spans entries
 * have.  A span's place in the output is closed form for KEEP and FILL and a 64-bit scan for DROP; one emit kernel writes the
 * piece's output in aligned 16-byte stores (st->pieces, rescans, max_carry: as acgpu_spans_stats).  Host output leaves through
 * the two slabs of the replace entries ("replace_slab_units").
 *  acgpu_cover_batch_u16 : many short texts in one call.  Haystack i is units[offsets[i] .. offsets[i + 1]) as for
 *              acgpu_match_batch_u16, empty haystacks allowed.  out[out_offsets[i] .. out_offsets[i + 1]) is, unit for unit, what
 *              acgpu_cover_u16 returns for haystack i alone with the same spec; the results lie back to back, out_offsets[0] == 0
 *              and *n_out == out_offsets[n_haystacks] (out_offsets: n_haystacks + 1 words in host memory).  More than cap units:
 *              ACGPU_E_OVERFLOW, *n_out and EVERY entry of out_offsets exact, nothing at or beyond out[cap] written.
 *              st->n_records and n_spans are sums over the haystacks.  ACGPU_E_INVALID, before a device is touched: NULL a,
 *              offsets, n_out, spec or out_offsets; descending offsets; a concatenation of 2^31 units or more; a cap without a
 *              buffer; what the spec checks above refuse.  n_haystacks == 0: ACGPU_OK, *n_out = 0, out_offsets[0] = 0, no
 *              device.  Works on the NULL stream under the pool's lock, tickets in flight are refused (STREAM RULE), as
 *              acgpu_replace_batch_u16.
 *              How: the haystacks are staged once as one text with a separator unit behind each and go through the pieces as
 *              acgpu_cover_u16's text does.  A span that ends at a separator and one that starts behind it have the separator's
 *              uncovered position between them, so they stay two spans with two opens -- where cover of the JOINED text
 *              ("..ab" ++ "ab..") gives one.  Behind a piece's merge its final spans and its separators become one item list; a
 *              separator is an item that emits nothing and skips one unit, so the results come out back to back, and every
 *              result's first unit is read off the plan on the device (one copy of out_offsets at the end).  The plan, a
 *              64-bit scan for every body here, runs in front of the piece's one wait: NO wait is added per piece.  Where
 *              there is no free separator unit, or a word matcher's table is not fold-consistent, every haystack runs as a
 *              text of its own under the one lock, open and close uploaded once (st->pieces then counts them all).
 *  acgpu_cover_batch_utf8, acgpu_cover_batch_utf8_lossy : the same for haystacks of BYTES, haystack i being
 *              bytes[offsets[i] .. offsets[i + 1]) of one buffer as for acgpu_match_batch_utf8 (offsets[0] need not be 0).
 *              out[out_offsets[i] .. out_offsets[i + 1]) is, byte for byte, what acgpu_cover_utf8 (_lossy) returns for haystack i
 *              alone; out_offsets[0] == 0, out_offsets[n_haystacks] == *n_out; on ACGPU_E_OVERFLOW *n_out and every offset are
 *              exact and nothing at or beyond out[cap] is written.  All five families, keywords with an unpaired surrogate
 *              included; fill is one ASCII byte per covered byte.  The checks come in this order, none needing a device: the
 *              arguments (NULL a, offsets, n_out, out_offsets; a cap without a buffer), the spec as for acgpu_cover_utf8, the
 *              offsets as for acgpu_match_batch_utf8 (bytes plus haystacks below 2^31).  A batch without a byte: ACGPU_OK, every
 *              offset 0, no device.  Strict, ill-formed input (a sequence cut by a haystack boundary is ill-formed):
 *              ACGPU_E_ENCODING plainly after the transcoder's one wait, ust->bad_haystack and first_bad exactly what
 *              acgpu_match_batch_utf8 reports for the buffer, *n_out = 0, out and out_offsets[1 ..] untouched, the stream idle.
 *              Lossy: never ACGPU_E_ENCODING; every haystack is decoded on its own, outside the spans the output is a
 *              byte-for-byte copy, stray bytes included, and inside a FILL span they are filled.
 *              How: the scan sees units with a separator behind every haystack, the caller's bytes have none.  Merge, plan and
 *              emit work on the bytes with one PHANTOM element behind every haystack (position = byte of the buffer + index of
 *              the haystack): no record covers a phantom, so spans never reach across a seam -- also not the widened records of
 *              a keyword with an unpaired surrogate, which may touch only in bytes; a phantom is an item that emits nothing
 *              and skips one element, exactly as the separator of acgpu_cover_batch_u16; only the emit's source knows that the
 *              phantoms are not in the buffer and subtracts the haystack's index, which is constant within a segment.  No
 *              wait is added per piece.  The fallback (no free separator unit; a word matcher's table that is not
 *              fold-consistent) validates the whole batch first, so what is refused does not depend on the route.
 * One long text in chunks: acgpu_stream_cover_u16 / _utf8 / _utf8_lossy below.
 * Not built: device-resident and multi-device forms, per-keyword open / close, a one-launch form for tiny batches, the Java
 * facade.  ACGPU_ABI_VERSION stays as it is.
 */
enum { ACGPU_COVER_KEEP = 0, ACGPU_COVER_FILL = 1, ACGPU_COVER_DROP = 2 };
typedef struct acgpu_cover_spec {
    const void *open;         /* open_len elements in HOST memory (NULL if open_len == 0)                    */
    uint32_t open_len;
    const void *close;        /* close_len elements in HOST memory (NULL if close_len == 0)                  */
    uint32_t close_len;
    uint32_t body;            /* ACGPU_COVER_KEEP, _FILL or _DROP                                            */
    uint32_t fill;            /* ACGPU_COVER_FILL: the element written once per covered element              */
} acgpu_cover_spec;
typedef struct acgpu_cover_stats {
    uint64_t n_records;       /* records merged == records the Set match call returns                        */
    uint64_t n_spans;         /* spans of the text                                                           */
    uint64_t units_out;       /* elements of the result (exact, also on ACGPU_E_OVERFLOW)                    */
    uint32_t pieces, rescans; /* as acgpu_count_stats                                                        */
    uint32_t max_carry;       /* as acgpu_spans_stats                                                        */
    uint32_t reserved;
} acgpu_cover_stats;   /* 40 bytes */
int acgpu_cover_u16(const acgpu_automaton *a, const uint16_t *haystack, uint64_t n_units, const acgpu_cover_spec *spec, uint16_t *out,
                    uint64_t cap, uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */);
int acgpu_cover_device(const acgpu_automaton *a, acgpu_shard *shard, const acgpu_cover_spec *spec, uint16_t *d_out, uint64_t cap,
                       uint64_t *n_out, void *stream, acgpu_cover_stats *st /* may be NULL */);
int acgpu_cover_batch_u16(const acgpu_automaton *a, const uint16_t *units, const uint64_t *offsets, uint32_t n_haystacks,
                          const acgpu_cover_spec *spec, uint16_t *out, uint64_t cap, uint64_t *out_offsets /* n_haystacks + 1 */,
                          uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */);
int acgpu_cover_utf8(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const acgpu_cover_spec *spec, uint8_t *out,
                     uint64_t cap, uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */, acgpu_utf8_stats *ust /* may be NULL */);
int acgpu_cover_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, uint64_t n_bytes, const acgpu_cover_spec *spec, uint8_t *out,
                           uint64_t cap, uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */,
                           acgpu_utf8_lossy_stats *ust /* may be NULL */);
int acgpu_cover_batch_utf8(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                           const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap, uint64_t *out_offsets /* n_haystacks + 1 */,
                           uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */, acgpu_utf8_batch_stats *ust /* may be NULL */);
int acgpu_cover_batch_utf8_lossy(const acgpu_automaton *a, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_haystacks,
                                 const acgpu_cover_spec *spec, uint8_t *out, uint64_t cap, uint64_t *out_offsets /* n_haystacks + 1 */,
                                 uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */, acgpu_utf8_lossy_stats *ust /* may be NULL */);

/*
 * Stream cover: acgpu_cover_u16 / acgpu_cover_utf8 / acgpu_cover_utf8_lossy for a text that arrives in chunks of any size and may be
 * longer than 2^31 elements -- mask, highlight or redact a log file chunk by chunk, for ALL FIVE families (ACGPU_MODE_ALL and, for
 * bytes, keywords with an unpaired surrogate included).  A stream opened with acgpu_stream_open is fed through ONE of these three
 * entries; the first feed of any kind, an empty one included, decides what the stream is, and every other entry then returns
 * ACGPU_E_INVALID (nine kinds in all).  "Element" below: a UTF-16 unit for acgpu_stream_cover_u16, a byte for the byte entries.
 *  result : let T be the concatenation of everything fed and R the Set records that acgpu_stream_feed / acgpu_stream_feed_utf8 /
 *           acgpu_stream_feed_utf8_lossy deliver for T over all feeds.  The concatenation of out[0 .. *n_out) over all feeds is the
 *           cover of T by the spans of R under spec (every span open ++ body ++ close, everything else copied), whatever the
 *           chunking.  For a fold-consistent word table that is element for element what acgpu_cover_u16 / _utf8 / _utf8_lossy
 *           return for T; over a word table that is not fold-consistent the STREAM's records are meant (the Readable loops).
 *  a feed : delivers the rewrite of T[done_before : done_after).  For a feed that is not final done_after = max(done_before, B),
 *           B the position before which no later record can start, by the carry rule of the spans merge applied to the feed's
 *           owned range: AhoCorasick and Shortest: owned end + 1 - max_keyword_len; Longest, WholeWord, WholeWordLongest:
 *           max(owned end, end of the feed's last record); bytes: that unit mapped to bytes, rounded down to a code-point
 *           boundary and never past the end of the decoded bytes (a held prefix is never delivered before the bytes that
 *           complete it).  final != 0 delivers everything.  So a feed that is not final withholds at most max_keyword_len + 1
 *           units (bytes: 4 * (max_keyword_len + 2) + 3) HOWEVER LONG A SPAN IS: "aa" on "aaaa..." is one span through every feed.
 *  a span that done_after cuts (position done_after - 1 is covered and the span's end is >= done_after; an end EQUAL to done_after
 *           counts, a later record may start exactly there and touch): its open and its body up to done_after are delivered now
 *           (DROP: no body), its close by the feed that sees it end -- as the first thing that feed delivers if nothing touched it
 *           after all -- and no second open is ever written.  The stream carries done (64 bits, global), whether it stands
 *           inside a span, and the spans the merge withheld (at most max_keyword_len / 2 + 2, global coordinates) on the host.
 *  spec   : as for the cover entries; uploaded by every feed, and the spec of the feed that emits applies.  Pass the same one.
 *  cap, *n_out : in elements.  ACGPU_E_OVERFLOW: nothing was committed, *n_out (and st->units_out) is the exact size of THIS feed's
 *           output, out[0 .. cap) is unspecified and nothing at or beyond cap has been written; call the SAME feed again.
 *  st     : may be NULL; this feed alone, st->units_out == *n_out, st->n_spans the spans whose OPEN this feed delivered (summed
 *           over the feeds: the spans of T); n_records, pieces, rescans, max_carry as for the cover entries.  ust (bytes): may be
 *           NULL, as acgpu_stream_feed_utf8 / _lossy fill it.
 *  ACGPU_E_INVALID, before any device is touched and with out, st and ust untouched: NULL s or n_out, data without a buffer, cap
 *           without out, a finished or detached stream, a stream of another kind, what the cover entries refuse about spec
 *           (NULL, body > 2, a NULL pointer with a length, 2^31 elements of open or close, a fill the element does not hold:
 *           bytes >= 0x80), n >= 2^31 or carried + n >= 2^31.  Tickets in flight on the pool: ACGPU_E_INVALID as well.
 *  ACGPU_E_UNSUPPORTED, before any device is touched: a pipelined stream.
 *  ACGPU_E_ENCODING (strict bytes): as acgpu_stream_replace_utf8 -- ust->first_bad is the GLOBAL offset, *n_out = 0, out untouched,
 *           the stream is finished, and what earlier feeds had withheld (a pending close included) is NOT delivered.
 *  no device : an empty feed that is not final; an empty final feed on a stream that holds nothing; and for acgpu_stream_cover_u16
 *           any empty final feed on a text already delivered to its end -- inside a span it delivers close, copied on the host
 *           from spec (the byte entries do the same where they carry no bytes, else they go through the device).
 * Device and lifetime as for acgpu_stream_feed.  Nothing of the stream lives on the device between two feeds, so any other call on
 * the automaton -- other streams and cover calls with other specs included -- may run between them.
 * How it works: a feed builds [carry | chunk] as the match feeds do and drives the pieces of the cover entries over its owned
 * range, scanned by the Readable rule, the merge starting from the spans the stream carries.  Inside a feed a span that is still
 * open at a piece's end is withheld as ever; the feed's last piece settles at B and emits the span it cuts there as a TAILLESS
 * item (no close), and the next feed emits the rest of it as a HEADLESS item (no open, body from done on) -- two kinds of item of
 * the one emit kernel, clipped in its source alone.  The carry always reaches back to done (keep_from = owned end - left context
 * never lies behind B); a feed that finds otherwise returns ACGPU_E_HIP.
 * Not built: a stream of spans (acgpu_stream_spans_*: the same state without the text), pipelined and reserved forms,
 * device-resident and multi-device forms, the Java facade.  ACGPU_ABI_VERSION stays as it is: adding symbols is compatible.
 */
int acgpu_stream_cover_u16(acgpu_stream *s, const uint16_t *units, uint64_t n_units, int final, const acgpu_cover_spec *spec,
                           uint16_t *out, uint64_t cap, uint64_t *n_out, acgpu_cover_stats *st /* may be NULL */);
int acgpu_stream_cover_utf8(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const acgpu_cover_spec *spec,
                            uint8_t *out, uint64_t cap, uint64_t *n_out, acgpu_utf8_stream_stats *ust /* may be NULL */,
                            acgpu_cover_stats *st /* may be NULL */);
int acgpu_stream_cover_utf8_lossy(acgpu_stream *s, const uint8_t *bytes, uint64_t n_bytes, int final, const acgpu_cover_spec *spec,
                                  uint8_t *out, uint64_t cap, uint64_t *n_out, acgpu_utf8_lossy_stream_stats *ust /* may be NULL */,
                                  acgpu_cover_stats *st /* may be NULL */);

/*
 * Synthetic haystack generator of the benchmark: unit i of the stream is
 * table[((z_i >> 32) * table_len) >> 32] with z_i = SplitMix64 output for counter
 * start_index + i of `seed` (see ahocorasick_amd/synth.py).  d_dst: device pointer.
 */
int acgpu_synth_fill(uint16_t *d_dst, uint64_t n_units, uint64_t start_index, uint64_t seed, const uint16_t *table,
                     uint32_t table_len, void *stream);

/*
 * Config 5's haystack (tokens -- a dictionary word with random per-unit case flips, or a random single-script
 * word -- separated by 1-3 separator units), generated in place on the device.  Token t owns draws 32 t .. 32 t + 31 of the
 * SplitMix64 stream `seed`, so the text is a function of (seed, dictionary) alone (ahocorasick_amd/synth.py:
 * token_stream_haystack is the numpy twin).  kw_units / kw_off / swapcase_tbl (65536 entries, may be NULL: no case flips) are
 * HOST pointers; d_dst is a device pointer.  Synchronises `stream`.
 */
int acgpu_synth_tokens(uint16_t *d_dst, uint64_t n_units, uint64_t seed, const uint16_t *kw_units, const uint64_t *kw_off,
                       uint32_t n_kw, const uint16_t *swapcase_tbl, void *stream);

/*
 * Measurement helper ("also report vs. a measured streaming-read kernel on the same box"): a pure read
 * of n_bytes (>= 1 MiB, 16-byte aligned device pointer), `repeats` timed launches after a warm-up (HIP events on `stream`,
 * synchronous), the median in *ms_median.
 *  pattern 1: the fastest pure read found on this chip (groups of 2 KiB tiles dealt round robin to small workgroups, 32 bytes
 *             per lane): the attainable ceiling bench.py reports next to the 8 TB/s spec peak;
 *  pattern 0: the access pattern of the tile kernels themselves -- every wave a contiguous span, 64 bytes per lane and tile,
 *             the next tile's loads in flight -- i.e. what their stream alone costs.
 */
int acgpu_stream_probe(const void *d_buf, uint64_t n_bytes, void *stream, int repeats, int pattern, float *ms_median);

/* tuning knobs: DEVELOPMENT AND TEST HOOK, not part of the product surface a JVM binds.  Process-wide, read when a call
 * is enqueued; set them only while no match call is running (each knob is a relaxed atomic, so a concurrent reader sees
 * the old or the new value, never a torn one, but a call may then mix settings).  name: "chunk_units",
 * "blocks_per_cu", "lds_table_bytes" (rows of the state x class table the DFA chunk scan keeps in LDS: default and maximum
 * 127 KB), "force_sparse", "dense_budget_bytes", "force_kernel" (0 auto, 1 DFA chunk
 * scan, 2 K-gram tile scan), "region_units", "filter_max_bytes", "ww_first_seed" (WHOLEWORD builder: index of the first
 * hash seed tried), and the builder's A/B switches "no_merged_ranges" (dictionaries over several ranges keep the class-table
 * filter), "no_short_keywords" (the filter's K stays at most the shortest keyword), "no_class_pages" (the class-table forms of
 * the tile kernel look classes up in global memory instead of LDS pages); "reserve_cus" (the scan kernels size their
 * grids for that many CUs fewer: a scan workgroup holds a whole CU's LDS, so k CUs stay free for the kernels of a collective
 * that runs under the scan -- RCCL's all-gather in a multi-GPU job); "tile_form" (bit 0: the K-gram tile scan leaves the
 * ordering of its records to a second kernel instead of its own tail, bit 1: the same for the WHOLEWORD kernel -- the
 * separate launches bench.py times beside the one-kernel call); the WHOLEWORD builder's and kernel's A/B switches
 * "ww_no_ph" (two-choice hash table instead of the perfect one), "ww_ph_lambda" (keys per bucket of the perfect hash,
 * default 4), "ww_no_byte_pages" (units staged as class codes, not as one byte each), "ww_block" (threads of a workgroup,
 * a multiple of 64) and "ww_ramp_pm" (per mille by which the spans of the last workgroups shrink); "longest_form" (bits:
 * 1 no k_longest_bits, 2 no k_longest_follow, 4 both for short texts too, 8 k_longest_follow over alphabets of up to four
 * letters); the cursor's "cursor_first_piece" (units of its first piece, default 2^20), "cursor_max_piece" (largest piece,
 * 2^26) and "cursor_reservoir_bytes" (largest reservoir, 256 MiB); "states_chunk_log2" (k_ac_states: a lane's chunk, 0 = by the text's
 * length, 8 .. 10 = forced) and the counting calls' A/B switches "count_form" (bits: 1 never the direct form, 2 no LDS counters
 * in k_states_hist, 4 no same-key peel in k_states_hist / k_count_ids); "replace_slab_units" (acgpu_replace_u16: units of one of the
 * two device slabs its result leaves through, default 2^25; it counts OUTPUT ELEMENTS, so for acgpu_replace_utf8 bytes; the cover entries' host output
 * leaves through the same slabs); "cover_lds_segments" (k_cover_emit: the segments of a tile it stages in LDS at most, default and
 * maximum 1536; 0 sends every tile through the global-memory view -- tests).  Returns the previous value, -1 for an unknown name. */
int64_t acgpu_set_tunable(const char *name, int64_t value);

const char *acgpu_strerror(int code);
int acgpu_last_hip_error(void);  /* hipError_t of the last ACGPU_E_HIP on this thread */
uint32_t acgpu_abi_version(void);

/* Test hook: copies the host-side tables of an automaton (NULL pointers are skipped).  Lets
 * CPU-only tests check the builder without a device.  dfa receives n_states*n_classes uint32
 * entries when info.dense, per-state arrays receive n_states entries. */
int acgpu_debug_tables(const acgpu_automaton *a, uint16_t *cls_lut /*65536*/, uint32_t *dfa, uint32_t *out_len,
                       uint32_t *out_link, uint32_t *out_id, uint32_t *depth, uint32_t *first_out_state);

/* Test hook (ACGPU_MODE_ALL / ACGPU_MODE_SHORTEST): the compact automaton k_ac_states walks (csrc/acgpu_build.cpp 6d), if the
 * dictionary has one (at most 255 classes, keywords of at most 32 units, fewer than 2^23 states).  sizes[6] is always written:
 * {states, states of the dense group, classes, words of rows, words of nodes, words of ids}; 0 states = none.  Arrays are copied
 * when the pointer is non-NULL: rows = dense-group rows of `classes` resolved transitions (target state | bit 23 "reports
 * matches" | its number of keywords << 24); nodes = 4 words per other state {fail state | 3 bits per edge: the child's number of
 * keywords (7 = more), then three edges class << 24 | bit 23 | child}; mask[state] = bit L - 1 per keyword length L ending there;
 * out = 2 words per state {mask, index of its keyword ids in ids -- or bit 31 | the id of its only keyword}; ids. */
int acgpu_debug_states(const acgpu_automaton *a, uint64_t sizes[6], uint32_t *rows, uint32_t *nodes, uint32_t *mask, uint32_t *out,
                       uint32_t *ids);

/* Test hook (ACGPU_MODE_WHOLEWORD, ACGPU_MODE_WWLONGEST): the whole-keyword hash table the device kernel probes.  Sizes and
 * the seed are always written; arrays are copied when the pointer is non-NULL.
 * Hashes of a folded keyword over its max(8, ceil(length/2)) packed words w (two units per word, zero beyond the keyword):
 *   h = seed; h = h*33 + w            ... then the murmur3 32-bit finaliser        (hash)
 *   g = seed; g = rotl(g, 5) ^ w                                                    (second hash)
 * slots: a two-choice table of n_slots (a power of two) slots of 8 uint32: {tag, id, units 0..11 packed two per word};
 * tag = (h & 0xffffff00) | min(length, 255), 0 = free slot; a keyword sits in slot (h & (n_slots-1)) or in slot
 * s2 = (((g ^ (h >> 16) ^ (g >> 13)) * 0x2C1B3C6D) >> 11) & (n_slots-1)  (s2 ^ 1 if that equals the first).  Keywords of
 * more than 12 units hold their record's offset (in 16-byte units) in place of the id.
 * recs: uint32 words, record = {keyword id, length, folded units packed two per word, zero padded to 16 bytes}.
 * fold_pgidx[256] / fold_pages[n_pages*256]: lower[u] = (u + fold_pages[fold_pgidx[u>>8]*256 + (u&255)]) & 0xffff;
 * page 0 is all zero.
 * ACGPU_MODE_WWLONGEST: the same table over the FIRST WORDS a walk can end or go on from -- the trie paths of word
 * characters only, of at most 12 units, that are a (trimmed, folded) keyword or go on with a non-word unit.  The id field
 * (and a record's first word) is then a payload: bit 31 set = the path goes on with a non-word unit, the low 31 bits are the
 * number of its trie node (the walk goes on from there, unit by unit); bit 31 clear = the walk ends on this keyword, the
 * payload is its id (the last one given, among duplicates).  No path of more than 12 units is in the table. */
int acgpu_debug_wordhash(const acgpu_automaton *a, uint32_t *n_slots, uint32_t *slots, uint64_t *n_rec_words, uint32_t *recs,
                         uint8_t *fold_pgidx, uint32_t *n_pages, uint16_t *fold_pages, uint32_t *seed);

/* Test hook (ACGPU_MODE_WHOLEWORD): what the position-parallel word kernel (k_ww_pp) probes in place of the two-choice table and
 * looks units up in.  sizes = {slots of the perfect hash, its buckets, byte pages}; 0 slots / 0 pages = not built.  Arrays are
 * copied when the pointer is non-NULL.
 * Perfect hash ("hash and displace") over the same hashes h, g as acgpu_debug_wordhash:
 *   bucket = (h * n_buckets) >> 32;  d = disp[bucket];
 *   t = (g ^ (h << 7)) + d * 0x9E3779B9;  t ^= t >> 15;  t *= 0x2C1B3C6D;  t ^= t >> 13;  slot = (t * n_slots) >> 32
 * every keyword sits in the slot its hashes name (slots: 8 uint32 each, the two-choice table's format); a run of word characters
 * that is no keyword reads some slot and fails the comparison of tag and units.
 * Byte pages (case-insensitive automata whose word-character table is fold-consistent): e = pages[idx[u >> 8] * 256 + (u & 255)];
 * word character = e & 1, lower[u] = (u + delta[e >> 1]) & 0xffff (delta: 128 entries). */
int acgpu_debug_wordhash_perfect(const acgpu_automaton *a, uint32_t sizes[3], uint32_t *slots, uint16_t *disp, uint8_t *bp_idx,
                                 uint8_t *bp_pages, uint16_t *bp_delta);

/* Test hook: the host's finishing pass of acgpu_count_batch_u16 on an entry list given by the caller -- no automaton, no device.
 * entries: 3 words {haystack, keyword_id, count} per entry, the haystacks never descending and below n_haystacks; the entries of
 * one haystack are sub-rows of ascending, distinct ids.  Out: the CSR matrix (row_ptr: n_haystacks + 1 entries; ids and counts:
 * room for n_entries), *n_terms its entries, *rows_cut the rows that had more than one sub-row and were sorted and merged.
 * ACGPU_E_HIP for a haystack index that descends or is out of range, with nothing written; ACGPU_E_INVALID for a NULL pointer. */
int acgpu_debug_count_batch_finish(const uint32_t *entries /* 3 per entry */, uint64_t n_entries, uint32_t n_haystacks, uint64_t *row_ptr,
                                   uint32_t *ids, uint32_t *counts, uint64_t *n_terms, uint32_t *rows_cut);

#ifdef __cplusplus
}
#endif
#endif /* ACGPU_H */
