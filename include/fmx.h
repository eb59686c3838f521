/*
 * fmx.h — C ABI of libfmx.so, the MI355X-native engine for index4j's backward-search path.
 *
 * This is the drop-in boundary.  index4j (pure Java) has no FFI seam of its own (FmIndex is a
 * final class), so the boundary is: the public FmIndex / FmIndexBuilder method
 * signatures on the host side, the serialized byte layout (FmIndex.write) as the hand-over format,
 * and the functions below as what a JNI / Panama binding of those methods calls.  Each function
 * cites the reference interface it replaces; paths are relative to
 * /root/reference/indices/src/main/java/com/dynatrace/ (FM = fm/FmIndex.java, FMB =
 * fm/FmIndexBuilder.java, SER = serialization/Serialization.java).
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function returns FMX_OK or a
 * negative library error (never throws).  Per-query failures (the reference's exceptions) are
 * reported in status[] with the FMX_ST_* codes so the host binding can re-throw the identical
 * exception type and message (fmx_status_message).  All batch calls run on the GPU; there is no CPU
 * query path in this library: without a HIP device they return FMX_E_NO_DEVICE.
 */
#ifndef FMX_H
#define FMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fmx_index fmx_index;

/* library-level return codes */
#define FMX_OK 0
#define FMX_E_ARG (-1)        /* bad argument */
#define FMX_E_ALPHABET (-2)   /* IllegalArgumentException("Input has more than 32767 different symbols") FM:423-426 */
#define FMX_E_FORMAT (-3)     /* malformed / truncated serialized stream */
#define FMX_E_VERSION (-4)    /* IOException("Incompatible serial versions! ...") SER:46-56 */
#define FMX_E_NO_DEVICE (-5)  /* no HIP device / index not resident on a device */
#define FMX_E_HIP (-6)        /* a HIP runtime call failed (see fmx_last_error) */
#define FMX_E_NOMEM (-7)
#define FMX_E_UNSUPPORTED (-8) /* e.g. text longer than one 2^32 hyperblock */

/* per-query status codes (exceptions of the reference; 0 = no exception) */
#define FMX_ST_OK 0
#define FMX_ST_NOT_ENABLED 1     /* RuntimeException "Text recovery not enabled at build time"   FM:566-568, 611-613 */
#define FMX_ST_POS_NEGATIVE 2    /* RuntimeException "Requested position less than 0"            FM:570-572, 615-617 */
#define FMX_ST_STOP_TOO_LONG 3   /* RuntimeException "Stop position longer than index string"    FM:574-576 */
#define FMX_ST_DEST_TOO_SMALL 4  /* RuntimeException "Supplied destination is not large enough"  FM:591-593 */
#define FMX_ST_POS_TOO_LONG 5    /* RuntimeException "Requested position longer than index string" FM:619-621 */
#define FMX_ST_DEST_SIZE_ZERO 6  /* IllegalArgumentException "Supplied destination for extraction has size zero" FM:623-625 */
#define FMX_ST_NO_BOUNDARY 7     /* IllegalArgumentException "Boundary does not exist"           FM:659-661, 792-794, 849-851 */
#define FMX_ST_DOES_NOT_FIT 8    /* RuntimeException "Extraction does not fit in the supplied destination. Currently extracted: N" (N in aux[]) FM:732-737, 816-821, 893-898 */
#define FMX_ST_JAVA_AIOOBE 9     /* the JVM would raise ArrayIndexOutOfBoundsException (e.g. empty pattern FM:456-457, locations[] too small FM:538) */
#define FMX_ST_TOO_MANY_RANGES 10 /* RuntimeError "Class pattern keeps more than max_ranges ranges" (the class calls only; no reference counterpart) */

/* ---- construction, persistence, lifetime ------------------------------------------------- */

/* new FmIndexBuilder().setSampleRate(s).setEnableExtraction(b).build(char[])  FMB:34-62 -> FM:155-174.
 * Host-side construction (suffix array, BWT, wavelet/RRR encoding); text = UTF-16 code units. */
int fmx_build(const uint16_t *text, int32_t n, int32_t sample_rate, int enable_extract, fmx_index **out);
/* The same index with the middle of the constructor computed on GPU `device`: FM:329-394 (suffix array by prefix
 * doubling, sampled rows, inverse samples, BWT) and FM:173 — the wavelet tree over the BWT (WFBB:130-154, 362-535,
 * 570-991) and its RRR vectors (RRR:225-286), encoded in HBM where the BWT lies (alphabets of up to 1,024 codes;
 * larger ones, and option "wavelet_on_device" = 0, encode the tree on the host).
 * The suffix array of a terminated text is unique and the encoders make the same choices, so the result is
 * byte-identical to fmx_build's (fmx_save gives the same bytes).  Optional statistics: doubling rounds after the initial 4-character sort, and rows
 * that went through a device sort, wall seconds of the device stage incl. transfers.  The handle still needs
 * fmx_to_device before queries. */
int fmx_build_on_device(const uint16_t *text, int32_t n, int32_t sample_rate, int enable_extract, int device,
                        fmx_index **out, int32_t *rounds, int64_t *rows_sorted, double *stage_seconds);
/* seconds fmx_build_on_device spent encoding the wavelet tree in HBM; 0 = it was encoded on the host */
double fmx_build_wavelet_seconds(const fmx_index *idx);

/* The suffix table of a resident index: fmx_to_device / fmx_attach_device_blob grow, level by level and with the very rank code the
 * queries run, the strings of 2, 3, ... codes that OCCUR in the text, each with its SA interval (the state of FM:455-474 after
 * a pattern's last characters), and hash ALL levels into one open-addressing table of 16-byte slots {key, start, end} (groups
 * of 64 slots, in-group slot = low bits of the first character's code XOR hash bits of the rest; at most 0.5 full, 0.7 where
 * only that keeps it inside its limit).  Depth *chars: as deep as a 64-bit key holds (8 codes of 8 bits, 4 of 16; option
 * "suffix_table_chars" caps it) while the table stays below the smaller of the budget (option "suffix_table_mb", default 256; 0
 * = no table) and 1 / "suffix_table_image_fraction" of the image (default an eighth).  Where the NEXT level exists but would
 * pass that limit as hashed slots, it is grown as CHILD LISTS if that fits the same limit (8-bit codes, at most 5 hashed
 * characters, "suffix_table_chars" permitting): a string X of that level is a string P of the deepest hashed level with one code
 * appended, and the X of one P lie side by side inside P's rows — so an X takes a code byte and its first row (five bytes,
 * its end is its neighbour's first row; a terminator per P), sorted under P's slot.  Such a level is complete or absent: every
 * string of *chars characters that the hashed form would hold is answered.  On the 256 MiB synthetic log: 5 characters hashed
 * in 8.4 MB, the 6th as lists, 19.7 MB together (limit 21.3).  count / locate batches start from the table: one slot (the
 * deepest level as lists: slot, codes, rows) instead of 2 * (k - 1) rank evaluations for a pattern's last k <= *chars
 * characters; a string that is not in it (it does not occur, holds an unknown character, or its search raised a status) is
 * searched by the loop.  Results, statuses and LF-step counts are unchanged (option "suffix_table" = 0 makes launches ignore
 * it, for A/B).  *chars = 0: no table; *bytes = the table's size, lists included (a power of two exactly when every level is
 * hashed). */
int fmx_suffix_table_info(const fmx_index *idx, int32_t *chars, int64_t *bytes);

/* The window directory of a resident index (grown by fmx_to_device / fmx_attach_device_blob beside the image, like the suffix
 * table; option "window_cells": 0 = none, 1 = always, in cells, 2 = the default rule: where it fits a quarter of the device's free
 * memory — and in its FLAT form where that costs at most 1/128 of the device's memory (option "window_flat_fraction"; 0 = never by
 * itself) and the alphabet has at most 2,048 symbols (the symbol search then runs in LDS), 3 = the flat form by name.  Flat = one 32-bit word per BWT position instead of cells and entries: every step of a walk is
 * ONE sector, at 4 bytes per text byte; locate 20-25 % faster, extract / extractUntilBoundary 10 %; texts below 2^30 characters.
 * Cells: one
 * 64-byte cell per 112 consecutive BWT positions holding, for the window's three most frequent symbols ("classes"), their folded
 * rank at the window start and — in two bit planes — the positions they stand at, plus every position's bit of sampledSuffixes
 * (FM:123) — and one entry per position that holds none of the three: everything the LF-step of that row hands back, whatever
 * route of the tree (and whichever of the reference's quirks) it takes.  An entry is 4 bytes for alphabets of up to 2,048 symbols
 * (the row the step arrives at; its symbol is the largest c with cumulativeCounts[c] < row, found by a search the kernels run in
 * LDS; the few answers that are more than a row — a status, a quirk — sit in 8-byte slots behind the entries) and 6 bytes beyond
 * {next row, symbol, status, suspect}; option "window_entry_bytes" = 4 / 6 forces a form (0, the default: by the alphabet).  An LF-step of
 * locate / extract / extractUntilBoundary — inverseSelect (WFBB:1305-1537) of a position, the poll of FM:531, the rank of FM:534 —
 * then costs ONE 64-byte sector, or two, and no walk through the wavelet tree, for EVERY row of the index (the tree's loop over
 * the levels of a code is what a 64-lane wave runs to the deepest code among its positions); count() does not use it.
 * 0.57 + 0.18 x 4 = 1.27 bytes per text byte on log text (1.65 with 6-byte entries).  Every number in it is the step the index's own rank() / inverseSelect()
 * took when the directory was grown: results, statuses and LF-step counts do not depend on having one.  Budget: option
 * "window_cells_mb" (default 65,536) caps it in absolute terms beside the quarter-of-free-memory rule of "window_cells" = 2;
 * fmx_resident_bytes says what an index took.  *bytes = its size (0: none). */
int fmx_window_cells_info(const fmx_index *idx, int64_t *bytes);
/* The row table of a resident FM-index (option "locate_rows", read when an index becomes resident: 0, the default, never;
 * 1 = for every index made resident afterwards whose text is shorter than 2^31 characters, where the table fits "window_cells_mb"
 * and a quarter of the device's free memory — the directory's two rules; any other value: FMX_E_ARG).  One 32-bit word per BWT
 * row beside the image (4 bytes per text character: the bytes of index4j's own sampleRate = 1 form, FM:343-344): WHAT locate()
 * RETURNS for a hit at that row (FM:538-542), written once per residency by the walk locate() itself runs for that row, over the
 * window directory where the index has one.  A pattern's hits are then end - start ADJACENT words: locate() — every entry point
 * that locates: fmx_locate_batch{,_dev}, fmx_locate_extract_batch, fmx_locate_lines_batch, the segment sets, the *_multi forms —
 * is the range search plus one gather, no LF-step.  Bit 31 of a word ("replay") marks the rows whose answer a word cannot carry
 * (the walk raised a status, or took a number of LF-steps other than value % sampleRate — a walk derailed by quirk Q1 may): those
 * hits are walked as without a table.  Positions, found counts, statuses and LF-step counts do not depend on having one.
 * The fill costs wt_size x sampleRate / 2 LF-steps per residency; a table that does not fit, or whose fill fails, is simply not
 * there (the index walks; not an error).  Never serialized.  RRR-only, wavelet-only and SuffixArray handles never get one.
 * *bytes = its size as allocated (0: none), *replay_rows = rows marked "replay" (each pointer nullable).
 * FMX_E_ARG for a null or SuffixArray handle. */
int fmx_locate_rows_info(const fmx_index *idx, int64_t *bytes, int64_t *replay_rows);
/* What a resident handle holds in its device's memory, in bytes (each pointer nullable): the image, the suffix table (with its
 * order-1 statistics), the window directory.  All 0 for a handle that is not resident.  (index4j's own figure for comparison is
 * the serialized size, FmIndexSerializedSizeBenchmark.java:57: 0.44-0.47 bytes per text byte.) */
int fmx_resident_bytes(const fmx_index *idx, int64_t *image, int64_t *suffix_table, int64_t *window_directory);

/* FmIndex.read(ObjectInput) FM:983-1025; also accepts the ObjectOutputStream-framed form produced by
 * Serialization.writeToByteArray SER:67-79 (magic AC ED 00 05 + block-data records). */
int fmx_load(const uint8_t *ser, size_t len, fmx_index **out);

/* FmIndex.write(ObjectOutput) FM:948-975; framed != 0 adds the SER:67-79 ObjectOutputStream framing.
 * *buf is owned by the library until fmx_free_buffer. */
int fmx_save(const fmx_index *idx, int framed, uint8_t **buf, size_t *len);
/* FM:956-960 writes the character map in java.util.HashMap's keySet() order, which fmx_save reproduces by replaying the map's
 * puts (capacity doubling, the resize a 9-node bucket forces below 64 slots, insertion order inside a bucket).  1 = that replay
 * covers this index; 0 = a JVM would have turned one of the buckets into a TREE bin (9 keys in one slot at 64 slots or more:
 * thousands of symbols whose codes collide modulo the table size), whose iteration order is not modelled — fmx_save's stream is
 * still one FmIndex.read accepts (its reader does not depend on the order, FM:992-998) but may differ from a JVM's bytes inside
 * that bucket; < 0 = error.  The Java shim reports it as GpuFmIndex.isSerializedFormVerified(). */
int fmx_save_key_order_modelled(const fmx_index *idx);
void fmx_free_buffer(uint8_t *buf);
void fmx_free(fmx_index *idx);

/* getInputLength FM:929 (includes the sentinel), getAlphabetLength FM:939, builder knobs FMB:21-22 */
int32_t fmx_input_length(const fmx_index *idx);
int32_t fmx_alphabet_length(const fmx_index *idx);
int32_t fmx_sample_rate(const fmx_index *idx);
int32_t fmx_extract_enabled(const fmx_index *idx);

/* ---- the flat HBM image ("blob") --------------------------------------------------------- */

/* Relocatable, pointer-free image of the whole index (layout: index4j_amd/csrc/fmx_blob.hpp).
 * It is what lives in HBM, and what is broadcast to the other GPUs over RCCL. */
int fmx_blob(const fmx_index *idx, const uint8_t **blob, size_t *len);
/* copy the blob into HBM of `device` (hipMalloc + hipMemcpy) and make idx queryable there */
int fmx_to_device(fmx_index *idx, int device);
/* adopt a blob that already sits in device memory (e.g. the receive buffer of an RCCL broadcast).
 * The memory stays owned by the caller and must outlive the index. */
int fmx_attach_device_blob(void *device_blob, size_t len, int device, fmx_index **out);
void *fmx_device_blob(const fmx_index *idx, size_t *len);

/* ---- batched queries: host buffers (H2D copy, kernels, D2H copy, synchronous) ------------- */

/* Optional: pin a long-lived host buffer of the caller (a direct ByteBuffer of the Java shim, a reused array) so that the
 * host-buffer entry points move it by DMA without staging copies; buffers that are not registered work all the same.
 * fmx_count_batch with ALL of its arrays registered copies nothing: one launch reads the patterns from the mapped arrays and
 * stores counts / LF-steps / statuses into them (option "host_mapped" = 0: the chunk pipeline instead; "host_direct_stores" = 0:
 * that pipeline with result copies).  Register WHOLE arrays: a kernel is only handed an array that lies inside ONE range
 * registered through THIS function (the library keeps the table; an array pinned some other way, or spanning two
 * registrations, takes the staged copies), and the HIP runtime refuses to copy a range registered only in part (FMX_E_HIP).
 * A registered array must stay registered, and must not be written by the caller, while a call that was given it is in
 * flight: the kernels read and write its pages directly, and the offsets are validated on the host before the launch.
 * (hipHostRegister / hipHostUnregister; pages stay locked until unregistered.) */
int fmx_host_register(void *p, size_t bytes);
int fmx_host_unregister(void *p);

/* int count(char[] pattern, int offset, int length) FM:455-474, batched: pattern i is
 * pat[pat_off[i] .. pat_off[i+1]).  lf_steps[i] (nullable) = number of C[c]+rank evaluations spent
 * (FM:469-470). status[i] (nullable) is FMX_ST_JAVA_AIOOBE for an empty pattern.
 * Batches of >= 131,072 patterns (option "host_pipeline_min") travel in chunks of 262,144 patterns, a chunk's transfer
 * overlapping the kernels of the one before; pat_off must start at >= 0 and never decrease (FMX_E_ARG otherwise).
 * Small calls — up to 2,048 patterns (option "host_small_max"; the same holds for fmx_locate_batch, fmx_extract_batch,
 * fmx_extract_boundary_batch, fmx_locate_extract_batch and fmx_locate_lines_batch): everything the call moves goes through one pinned block the kernels read and write where it lies
 * (no copy calls): a batch of ONE — a Java caller's count(char[]) — costs ~25 us (locate ~50, extract of 64 characters ~70). */
int fmx_count_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                    int32_t *counts, int32_t *lf_steps, int32_t *status);

/* int locate(char[] pattern, int offset, int length, int[] locations, int maxMatches) FM:504-552.
 * locs is n rows of loc_cap ints (the caller's `locations` arrays); found[i] = return value =
 * number located (<= max_matches; max_matches = -1: unlimited, FM:488).  Hits are SA rows
 * start+1.. in order (FM:527-547), exactly the ones the reference returns. */
int fmx_locate_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                     int32_t max_matches, int32_t *locs, int32_t loc_cap, int32_t *found, int32_t *lf_steps,
                     int32_t *status);

/* int locate(char[] pattern, int[] locations) FM:487-489, "all occurrences" (FM:487-552), batched and PACKED — the host form of
 * fmx_locate_all_ranges_dev + fmx_locate_all_fill_dev (below: the layout, max_matches, what lf_steps / status hold).
 * host buffers, synchronous: hit_off = n + 1 int64 (out); *locs = hit_off[n] ints owned by the library until
 * fmx_free_buffer((uint8_t *)*locs) (NULL when there are no hits); lf_steps / status nullable, n ints.
 * The hits of pattern i are (*locs)[hit_off[i] .. hit_off[i + 1]), in the order locate() stores them.  Device scratch is bounded:
 * the hits come down in windows of 2^24.  n == 0: FMX_OK, hit_off[0] = 0, *locs = NULL.  FMX_E_NOMEM if the result cannot be
 * allocated (nothing is left behind; *locs = NULL on every failure); FMX_E_ARG for null or negative arguments, pattern offsets
 * that start below 0 or decrease, and a SuffixArray, RrrVector or stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that
 * is not resident.  When every pattern has a few hits at most, fmx_locate_batch with a small loc_cap is the faster form (it
 * orders the walks; README). */
int fmx_locate_all_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_matches,
                         int64_t *hit_off, int32_t **locs, int32_t *lf_steps, int32_t *status);

/* THE LINES THAT MATCH: which lines hold each pattern, every line once, in text order (grep -n), how many (grep -c), the first
 * max_lines of them (grep -m) — the host form of fmx_locate_all_ranges_dev + fmx_locate_all_fill_dev (every hit, no limit) +
 * fmx_lines_of_hits_dev (below: the line table, what a line is).  Needs a line table (fmx_line_table_build).
 * host buffers, synchronous: line_off = n + 1 int64 (out), the exclusive sum of max_lines > 0 ? min(line_count, max_lines) :
 * line_count (max_lines -1 and 0: every line); *lines = line_off[n] ints owned by the library until
 * fmx_free_buffer((uint8_t *)*lines) (NULL when there are none): (*lines)[line_off[i] .. line_off[i + 1]) = the distinct line ids
 * of pattern i, ascending — with a limit the smallest max_lines of them; line_count[i] (nullable) = ALL distinct lines of pattern
 * i whatever the limit; occurrences[i] (nullable) = count(); status[i] (nullable) as fmx_locate_all_batch leaves it (an empty
 * pattern: FMX_ST_JAVA_AIOOBE and no lines).  What comes down from the device is the lines, not the hits: " " occurs 30,094 times
 * in the 2,000 lines of the reference's log fixture.  Device scratch grows with the batch's hits, no windows in this version —
 * 32 bytes per hit (positions 4, lines 4, fmx_lines_of_hits_dev's workspace 24) plus the radix sort's temporary storage, about
 * one more 8-byte key per hit, each block rounded up to a power of two: FMX_E_NOMEM when it, or the result, cannot be allocated (nothing is left behind; *lines = NULL on every
 * failure).  FMX_E_ARG as fmx_locate_all_batch, for an index without a line table (fmx_last_error names fmx_line_table_build),
 * and for a batch of more than 2^31 - 1 hits; FMX_E_NO_DEVICE for a handle that is not resident. */
int fmx_match_lines_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_lines,
                          int64_t *line_off, int32_t **lines, int32_t *line_count, int32_t *occurrences, int32_t *status);
/* [start[i], stop[i]) of line lines[i], the boundary excluded — what fmx_extract_batch takes; an id outside [0, n_lines) gets
 * start = stop = -1.  Host buffers, synchronous.  FMX_E_ARG without a line table. */
int fmx_line_bounds_batch(const fmx_index *idx, const int32_t *lines, int32_t n, int32_t *start, int32_t *stop);

/* THE LINES THAT MATCH A QUERY OF SEVERAL TERMS — the host form of fmx_locate_all_ranges_dev + fmx_locate_all_fill_dev (every
 * hit, no limit) + fmx_query_lines_of_hits_dev (below: what a query is, the rules, the key-width limit).  The batch holds n
 * TERMS, packed as everywhere (pat, pat_off), cut into q queries by query_off (q + 1 ints, query_off[0] = 0, never decreasing,
 * query_off[q] = n); term_kind[t] = FMX_TERM_ALL, FMX_TERM_ANY or FMX_TERM_NONE.  Needs a line table (fmx_line_table_build).
 * host buffers, synchronous: line_off = q + 1 int64 (out), the exclusive sum of max_lines > 0 ? min(line_count, max_lines) :
 * line_count (max_lines -1 and 0: every line); *lines = line_off[q] ints owned by the library until
 * fmx_free_buffer((uint8_t *)*lines) (NULL when there are none, and on every failure): (*lines)[line_off[Q] .. line_off[Q + 1]) =
 * the line ids of query Q, ascending, each once — with a limit the smallest max_lines of them; line_count[Q] (nullable, q
 * entries) = ALL lines of query Q whatever the limit; occurrences[t] (nullable, n entries) = count() of term t; status[t]
 * (nullable, n entries) as fmx_locate_all_batch leaves it (an empty pattern: FMX_ST_JAVA_AIOOBE and no hits — as an ALL term it
 * empties its query, as a NONE term it filters nothing).  q queries of ONE ALL term each give, array for array, what
 * fmx_match_lines_batch gives for those patterns.  What comes down from the device is the lines of the QUERIES, not the hits
 * and not the lines of the terms.  Device scratch grows with the batch's hits, no windows in this version: 48 bytes per hit
 * (positions 4, lines 4, fmx_query_lines_of_hits_dev's workspace 40) plus rocPRIM's temporary storage: FMX_E_NOMEM when it, or
 * the result, cannot be allocated.  FMX_E_ARG for null or negative arguments, a query_off that does not start at 0, decreases
 * or does not end at n, a kind above 2, an index without a line table (fmx_last_error names fmx_line_table_build), a batch of
 * more than 2^31 - 1 hits, a key of more than 64 bits, a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE
 * for a handle that is not resident.  n == 0 with q > 0 (queries without terms) is a batch like any other: no lines. */
#define FMX_TERM_ALL 0
#define FMX_TERM_ANY 1
#define FMX_TERM_NONE 2
int fmx_match_query_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int32_t *query_off,
                          const uint8_t *term_kind, int32_t q, int32_t max_lines, int64_t *line_off, int32_t **lines,
                          int32_t *line_count, int32_t *occurrences, int32_t *status);

/* PATTERNS OF CHARACTER CLASSES (grep -i, [0-9]) — the host forms of fmx_class_ranges_count_dev + fmx_class_ranges_fill_dev and what
 * follows them (below: what a class pattern is, its ranges, the statuses, max_ranges).  A batch is three packed arrays, one level
 * more than the literal calls take: alt = UTF-16 code units; pos_off = n_pos + 1 ints, never decreasing: position j has the
 * alternatives alt[pos_off[j] .. pos_off[j + 1]); pat_off = n + 1 ints, never decreasing, indexing POSITIONS: pattern i is positions
 * pat_off[i] .. pat_off[i + 1).  The answer of pattern i is the union of the reference's answers for the distinct literal strings
 * it spells.  Host buffers, synchronous.
 * fmx_count_class_batch: counts[i] (n ints) = the sum of count() over those strings; status nullable, n ints.
 * fmx_locate_all_class_batch: hit_off = n + 1 int64 (out); *locs = hit_off[n] ints owned by the library until
 * fmx_free_buffer((uint8_t *)*locs) (NULL when there are no hits, and on every failure): the hits of pattern i, its ranges ascending
 * by SA row and inside a range the order fmx_locate_all_fill_dev stores — every literal's locate() list, intact.  The hits come down
 * in windows of 2^24, like fmx_locate_all_batch's.  status (nullable) has the walks' statuses folded in.
 * fmx_match_query_class_batch: the TERMS are class patterns; query_off, term_kind, q, max_lines, line_off, *lines, line_count,
 * occurrences and status as fmx_match_query_batch (q queries of ONE ALL term each are the match_lines of class patterns).  A term
 * with FMX_ST_TOO_MANY_RANGES has no hits.  Needs a line table.
 * All three: FMX_E_ARG for null or negative arguments, offsets that start below 0 or decrease, pat_off[n] above n_pos, max_ranges
 * outside [1, FMX_CLASS_RANGES_MAX], more than 2^31 - 1 ranges in one batch, and a SuffixArray, RrrVector or stand-alone wavelet
 * handle (the query form: as fmx_match_query_batch besides); FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM when
 * scratch or the result cannot be allocated.  Nothing is left behind on failure.  n == 0: FMX_OK, the offsets' first entry 0. */
#define FMX_CLASS_RANGES_MAX 1024
#define FMX_CLASS_ALTS_MAX 64
int fmx_count_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                          int32_t n, int32_t max_ranges, int32_t *counts, int32_t *status);
int fmx_locate_all_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                               int32_t n, int32_t max_ranges, int64_t *hit_off, int32_t **locs, int32_t *status);
int fmx_match_query_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                int32_t n, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t *line_count, int32_t *occurrences,
                                int32_t *status);

/* THE LINES THAT HOLD A SEQUENCE OF TERMS IN ORDER (grep 'A.*B') — the host forms of the two packed stages (literal or class
 * patterns, every hit, no limit) + fmx_sequence_lines_of_hits_dev (below: what a sequence is, the rule, the spans).  The batch
 * holds n TERMS, packed as everywhere, cut into q SEQUENCES by query_off (q + 1 ints, the rule of fmx_match_query_batch); the
 * terms of a sequence must occur on the line in the order they stand in the batch, without overlap.  The length of a term is
 * pat_off[t + 1] - pat_off[t]: its characters (literal) or its positions (class).  Needs a line table (fmx_line_table_build).
 * line_off = q + 1 int64 (out); *lines = line_off[q] ints owned by the library until fmx_free_buffer((uint8_t *)*lines) (NULL
 * when no line matches, and on every failure): the line ids of sequence Q, ascending, each once — with a limit the smallest
 * max_lines of them; line_count[Q] (nullable, q entries) = ALL lines of sequence Q whatever the limit; occurrences[t] and
 * status[t] (nullable, n entries) per TERM as in fmx_match_query_batch (an empty term: status 9, no hits — its sequence has no
 * lines).  spans (nullable): *spans = *lines + line_off[q], 2 * line_off[q] ints IN THE SAME ALLOCATION behind the lines (free
 * *lines only; NULL when *lines is): {span_start, span_stop} of every stored line, in the order of *lines.
 * A ONE-TERM sequence is fmx_match_lines_batch of that term LESS the hits that run over the line's end: the pattern "\n" (the
 * boundary) has no lines here, and a pattern that holds the boundary matches nowhere.
 * Errors as fmx_match_query_batch (no kinds, no key-width limit: the key term | position always fits). */
int fmx_match_sequence_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int32_t *query_off,
                             int32_t q, int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t **spans, int32_t *line_count,
                             int32_t *occurrences, int32_t *status);
int fmx_match_sequence_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                   const int32_t *pat_off, int32_t n, int32_t max_ranges, const int32_t *query_off, int32_t q,
                                   int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t **spans, int32_t *line_count,
                                   int32_t *occurrences, int32_t *status);

/* THE VALUES THAT FOLLOW A PATTERN, WITH COUNTS (grep -o 'blk_[^ ]*' | sort | uniq -c; a terms aggregation) — the host forms of the
 * two packed stages (literal or class patterns, every hit, no limit) + fmx_values_of_hits_dev / fmx_values_fill_dev (below: the
 * definition of a value, the order, the stages).  One stop set (n_stop UTF-16 code units, 0 .. 64, duplicates allowed) and one
 * max_len in [1, 64] for the batch.  The length of a pattern is pat_off[i + 1] - pat_off[i]: its characters (literal) or its
 * positions (class).  No line table is needed.
 * val_off = n + 1 int64 (out), val_off[0] = 0: the values of pattern i are val_off[i] .. val_off[i + 1] - 1, ascending by UTF-16
 * code unit, a value in front of its extensions; G = val_off[n].  The result is ONE allocation owned by the library until
 * fmx_free_buffer((uint8_t *)*counts): *counts = G ints, the hits that have each value (the counts of a pattern add up to its
 * hits); *text_off = G + 1 int64 and *chars = (*text_off)[G] code units point INTO that allocation (free *counts only): value g is
 * (*chars)[(*text_off)[g] .. (*text_off)[g + 1]).  All three are NULL when there are no values, and on every failure.
 * occurrences[i] and status[i] (nullable, n entries) per pattern as in fmx_match_lines_batch: an empty pattern keeps
 * FMX_ST_JAVA_AIOOBE and has no values; on an index built without extraction every pattern gets FMX_ST_NOT_ENABLED and no values
 * (occurrences is still filled); a class pattern with FMX_ST_TOO_MANY_RANGES has none either.  Values are never merged across
 * patterns.  Only the groups come down: the hits and their windows stay on the device.  Device scratch grows with the HITS, no
 * windows over the answer in this version: 4 bytes per hit for the positions, 12 for the groups' counts and offsets, and
 * fmx_values_of_hits_scratch_bytes (about 170 + 2 * max_len per hit).  FMX_E_NOMEM when the scratch or the result cannot be
 * allocated (nothing is left behind); FMX_E_ARG for null or negative arguments, max_len or n_stop outside their intervals, more
 * than 2^31 - 1 hits or hits * max_len above 2^35, and a SuffixArray, RrrVector or stand-alone wavelet handle; FMX_E_NO_DEVICE for
 * a handle that is not resident.  n == 0: FMX_OK, val_off[0] = 0. */
int fmx_field_values_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *stop,
                           int32_t n_stop, int32_t max_len, int64_t *val_off, int32_t **counts, int64_t **text_off, uint16_t **chars,
                           int32_t *occurrences, int32_t *status);
int fmx_field_values_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                 const int32_t *pat_off, int32_t n, int32_t max_ranges, const uint16_t *stop, int32_t n_stop,
                                 int32_t max_len, int64_t *val_off, int32_t **counts, int64_t **text_off, uint16_t **chars,
                                 int32_t *occurrences, int32_t *status);

/* THE VALUES THAT FOLLOW A PATTERN, WHERE THE LINE MATCHES A QUERY (grep terminating | grep -o 'blk_[^ ]*' | sort | uniq -c; the
 * "count by" of a log search, which always carries a filter and a time window) — fmx_field_values_batch over the hits that lie in
 * given lines: the two packed stages over ONE batch of the filter terms and the value patterns + fmx_query_lines_of_hits_dev over
 * the terms' hits (no limit) + fmx_hits_in_lines_dev over the value patterns' hits (below: the keep rule) + the values stages over
 * the kept hits.  Nothing in between comes down: neither the lines nor the hits.
 * The n VALUE PATTERNS are (pat, pat_off, n); the n_terms TERMS (term_pat, term_off, n_terms) are cut into q queries by query_off /
 * term_kind exactly as in fmx_match_query_batch, whose definitions hold unchanged: a query of NONE terms only has no lines, so a
 * value pattern that asks for it has no values; a term with FMX_ST_TOO_MANY_RANGES has no hits, as in fmx_match_query_class_batch.
 * where_of = n ints, each -1 .. q - 1: a hit of pattern i counts iff its line — the line of its FIRST character — lies in
 * [line_lo, line_hi) and, for where_of[i] >= 0, belongs to query where_of[i]; several patterns may share a query.  A window of 0,
 * INT32_MAX does not filter.  A line table (fmx_line_table_build) is needed only if some where_of[i] >= 0 or a window is given;
 * with every where_of[i] < 0 and no window the answer is bit for bit fmx_field_values_batch's.
 * stop, n_stop, max_len, val_off, *counts, *text_off, *chars and status: fmx_field_values_batch's, the ONE allocation included (free
 * *counts only; all three NULL when there are no values and on every failure).  occurrences[i] (nullable) stays the pattern's
 * count in the WHOLE text; kept[i] (nullable, n ints) is the hits that passed: the counts of pattern i's values add up to kept[i]
 * (it is filled on an index built without extraction too, where every status is FMX_ST_NOT_ENABLED and there are no values).
 * term_status (nullable, n_terms ints) carries the terms' statuses, as fmx_match_query_batch's status does.
 * Device scratch: 4 bytes per hit of the merged batch, the query stage's over the TERMS' hits, the filter's 8 bytes per hit, and the
 * values stage's about 170 + 2 * max_len bytes per KEPT hit only.  One more 8-byte-per-pattern read and wait than
 * fmx_field_values_batch: the kept hits' offsets come down before the values stage is sized.
 * FMX_E_ARG for null or negative arguments, line_lo > line_hi, a where_of outside -1 .. q - 1, query_off / term_kind that
 * fmx_match_query_batch refuses, offsets that decrease, max_len or n_stop outside their intervals, an index without a line table
 * when the call filters (the error names fmx_line_table_build), more than 2^31 - 1 hits in the merged batch, a SuffixArray,
 * RrrVector or stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM as
 * fmx_field_values_batch.  n == 0: FMX_OK, val_off[0] = 0, nothing is searched and term_status is zeroed. */
int fmx_field_values_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                 const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint16_t *stop, int32_t n_stop,
                                 int32_t max_len, int64_t *val_off, int32_t **counts, int64_t **text_off, uint16_t **chars,
                                 int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status);
/* ... with class patterns as value patterns (alt, pos_off, n_pos, pat_off, n) and as terms (term_alt, term_pos_off, term_n_pos,
 * term_off, n_terms): the three packed arrays of fmx_count_class_batch, twice; one max_ranges for both. */
int fmx_field_values_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                       const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                       const uint8_t *term_kind, int32_t q, const int32_t *where_of, int32_t line_lo, int32_t line_hi,
                                       const uint16_t *stop, int32_t n_stop, int32_t max_len, int64_t *val_off, int32_t **counts,
                                       int64_t **text_off, uint16_t **chars, int32_t *occurrences, int32_t *kept, int32_t *status,
                                       int32_t *term_status);

/* LINES AND HITS PER BUCKET OF LINES (the timeline of a log search: the matching events per time bucket, beside the hit list and
 * the "count by") — the host forms of fmx_lines_histogram_dev and fmx_hits_histogram_dev (below: the stages).
 * EDGES: edges = n_edges >= 2 ints, B = n_edges - 1 buckets.  They are line ids, in the ids of fmx_line_bounds_batch; edges[0] >= 0;
 * they never decrease, equal neighbours make an empty bucket; they may exceed the number of lines.  Bucket b is the lines L with
 * edges[b] <= L < edges[b + 1]; a line below edges[0] or at or above edges[B] is counted in no bucket.  One edge array serves the
 * whole batch.  (Edges come from timestamps with what exists: the first line that holds "081109 2035" is
 * fmx_match_lines_batch's first line for it, max_lines = 1.)  Counts are int32; (int64) rows * B above 2^27 is FMX_E_ARG.
 * LINES PER BUCKET: hist = the caller's q * B ints, hist[Q * B + b] = the number of lines of query Q in bucket b — the lines are
 * fmx_match_query_batch's, whose definitions (pat, pat_off, n, query_off, term_kind, q; line_count, occurrences, status, each
 * nullable) hold unchanged: a query of NONE terms only has no lines, so a row of zeros; row Q adds up to line_count[Q] when the
 * edges span every line.  The two packed stages, fmx_query_lines_of_hits_dev (no limit) and fmx_lines_histogram_dev run; only hist
 * and the small per-query and per-term arrays come down — the lines do not.
 * FMX_E_ARG as fmx_match_query_batch, and for n_edges < 2, a negative first edge, decreasing edges, more than 2^27 counters;
 * FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing behind.  n == 0: FMX_OK, hist and line_count are
 * zeroed, nothing is searched. */
int fmx_line_histogram_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int32_t *query_off,
                             const uint8_t *term_kind, int32_t q, const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *line_count,
                             int32_t *occurrences, int32_t *status);
/* ... with class patterns as terms: the three packed arrays of fmx_count_class_batch and max_ranges, as fmx_match_query_class_batch */
int fmx_line_histogram_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                   int32_t n, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                   const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *line_count, int32_t *occurrences,
                                   int32_t *status);
/* HITS PER BUCKET: fmx_field_values_where_batch's call without the values stage (its value patterns, terms, query_off, term_kind,
 * where_of, occurrences, kept, status and term_status, no window).  hist = the caller's n * B ints, hist[i * B + b] = the number of
 * hits of value pattern i that fmx_hits_in_lines_dev keeps for where_of[i] and whose line — the line of the hit's FIRST character
 * — lies in bucket b.  A hit is counted as often as it occurs: two "blk_" on one line are two.  Row i adds up to at most kept[i],
 * and to exactly kept[i] when the edges span every line.  With every where_of[i] < 0 the filter stage is skipped and the raw hits
 * are binned (kept[i] = occurrences[i]).  A line table is needed in every case: the buckets are lines.
 * FMX_E_ARG as fmx_field_values_where_batch (its window, stop set and max_len aside) and for the edges as above, an index without a
 * line table (the error names fmx_line_table_build); FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing
 * behind.  n == 0: FMX_OK, nothing is searched and term_status is zeroed. */
int fmx_hit_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                  const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                  const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t *hist, int32_t *occurrences,
                                  int32_t *kept, int32_t *status, int32_t *term_status);
/* ... with class patterns as value patterns and as terms, as fmx_field_values_where_class_batch */
int fmx_hit_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                        int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                        const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                        const uint8_t *term_kind, int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges,
                                        int32_t *hist, int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status);

/* THE NUMBER BEHIND A PATTERN: STATISTICS PER BUCKET OF LINES (stats sum(size) p95(size) by minute where line has addStoredBlock:
 * "how much" beside the timeline's "how many") — the host forms of fmx_numbers_of_hits_dev (below: the stage).
 * THE VALUE OF A HIT: with len the length of the hit's pattern and textLength = fmx_input_length - 1, the hit's window is
 *     s = min(max(h + len, 0), textLength),   e = min(s + 32, textLength)
 * (fmx_field_values_batch's window at max_len = 32); its text is what extract(s, e, destination, 0) stores.  Over the window's
 * code units, with F = frac_digits in [0, 9]: D = the maximal run of '0' .. '9' at the window's start; D == 0 is NOT A NUMBER,
 * D == 32 is OVERFLOW (the run fills the window and may go on).  With F > 0 and '.' behind the run, up to F digits behind it are
 * the fraction, k of them; further digits are ignored (truncation, no rounding); without a '.', or with F == 0, k = 0.
 *     value = int(run) * 10^F + int(fraction) * 10^(F - k)      ("12.5" at F = 0 is 12, "1." at F = 3 is 1000, "251.73" 251730)
 * value > 2^63 - 1 is OVERFLOW.  There is no sign, no exponent and no thousands separator: the pattern "blk_-" reads the digits
 * behind a minus.
 * THE ROWS: fmx_hit_histogram_where_batch's call (its value patterns, terms, query_off, term_kind, where_of, edges, occurrences,
 * kept, status and term_status) with one addition: edges == NULL with n_edges == 0 means B = 1, every line — then no line table is
 * needed unless a pattern asks for a query.  Per row = i * B + b, over the kept hits of value pattern i whose line lies in bucket
 * b and that parse: count[row] (int32); sum_lo[row], sum_hi[row] (uint64): the exact sum = sum_hi * 2^64 + sum_lo; min[row],
 * max[row] (int64), 0 where count is 0; pct[row * P + j] (int64), P = n_permille in [0, 16], permille[j] in [0, 1000]: the
 * nearest-rank percentile — with c = count[row] the element of the ascending values at index max(1, ceil(permille[j] * c / 1000))
 * - 1, in 64-bit integer arithmetic; 0 where c is 0; permille 0 is the min, 1000 the max.  Per pattern: not_number[i], overflow[i]
 * (int32) = the kept hits IN SOME BUCKET that did not parse, by reason.  For every i
 *     sum over b of count[i * B + b] + not_number[i] + overflow[i] = the total of row i of fmx_hit_histogram_where_batch
 * for the same call.  Every output is nullable except count.  On an index built without extraction every status is
 * FMX_ST_NOT_ENABLED, all rows and counters are zero, occurrences and kept are still filled.  A window the packed extract ran
 * literally hands its status to its pattern, as in fmx_field_values_batch.
 * The packed stages up to the filter run as for the hits histogram (skipped with every where_of[i] < 0), then
 * fmx_numbers_of_hits_dev over the kept hits: about 150 bytes of scratch per kept hit (fmx_numbers_of_hits_scratch_bytes), and no
 * wait beyond the hits histogram's own — the rows have a known size.  Only the rows and the small per-pattern and per-term arrays
 * come down.
 * FMX_E_ARG as fmx_hit_histogram_where_batch (an index without a line table: only when edges are given or a pattern asks for a
 * query) and for frac_digits outside [0, 9], n_permille outside [0, 16], a permille outside [0, 1000], (int64) n * B above 2^27,
 * n * B * max(P, 1) above 2^27; FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing behind.  n == 0:
 * FMX_OK, nothing is searched and term_status is zeroed. */
int fmx_number_stats_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                 const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille,
                                 int32_t n_permille, int32_t *count, uint64_t *sum_lo, uint64_t *sum_hi, int64_t *min, int64_t *max,
                                 int64_t *pct, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                 int32_t *term_status);
/* ... with class patterns as value patterns and as terms, as fmx_hit_histogram_where_class_batch; a position is one character of
 * the pattern's length */
int fmx_number_stats_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                       const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                       const uint8_t *term_kind, int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges,
                                       int32_t frac_digits, const int32_t *permille, int32_t n_permille, int32_t *count, uint64_t *sum_lo,
                                       uint64_t *sum_hi, int64_t *min, int64_t *max, int64_t *pct, int32_t *not_number, int32_t *overflow,
                                       int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status);

/* THE LINES RANKED BY THE NUMBER BEHIND A PATTERN (... | sort -k latency -nr | head -10: "show me the ten slowest requests") — the
 * host forms of fmx_top_lines_of_hits_dev (below: the stage).  For number pattern i of the n value patterns:
 * THE KEPT HITS are exactly fmx_number_stats_where_batch's without edges (its value patterns, terms, query_off, term_kind, q and
 * where_of), further cut by the window of lines line_lo <= L < line_hi of fmx_field_values_where_batch (0 .. INT32_MAX: every
 * line).  A hit belongs to the line of its first character.
 * THE VALUE OF A HIT is fmx_number_stats_where_batch's, bit for bit (the window of 32 code units behind the pattern, ONE
 * frac_digits in [0, 9] per call).  Only the hits that parse take part; the others are counted per pattern as not_number[i] and
 * overflow[i].
 * THE ORDER: descending[i] (one byte per pattern): 1 is largest first, 0 smallest first.
 * THE CANDIDATE OF A LINE is the kept parsing hit on it that ranks best in that order; among hits of equal value the smallest
 * text position wins.  A line without a parsing kept hit has no candidate.
 * THE RANKING: the candidates of pattern i ordered by value in the order asked, equal values by ascending line id — a total order,
 * a line has one candidate.  lines[i] = the candidates, numbers[i] = the parsing kept hits, so
 *     numbers[i] + not_number[i] + overflow[i] = kept[i].
 * THE ROWS: first >= 0 and top >= 1 hold for the whole call; the rows of pattern i are the ranks first .. first + top - 1:
 * rows[i] = min(top, max(0, lines[i] - first)).  Row (i, j) lives at i * top + j: row_line (int32), row_value (int64), row_loc
 * (int32: the candidate's position); the entries at j >= rows[i] are stored as 0.  Every output is nullable except rows.
 * occurrences, kept, status and term_status as in fmx_number_stats_where_batch.  On an index built without extraction every
 * status is FMX_ST_NOT_ENABLED, all rows and counters are zero, occurrences and kept are still filled.  A window the packed
 * extract ran literally hands its status to its pattern.  The terms are plain strings: a ranged term (fmx_match_query_number_batch)
 * is not taken yet.
 * The packed stages up to the filter run as for the number statistics (skipped when nothing filters), then
 * fmx_top_lines_of_hits_dev over the kept hits; when no value pattern has a hit nothing is launched for the stage.  Only the
 * n x top rows and the small per-pattern and per-term arrays come down, never the hits.
 * FMX_E_ARG as fmx_number_stats_where_batch and fmx_field_values_where_batch judge their arguments, for frac_digits outside [0, 9],
 * first < 0, top < 1, (int64) n * top above 2^27, and ALWAYS for an index without a line table (the answer is lines);
 * FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing behind.  n == 0: FMX_OK, nothing is searched and
 * term_status is zeroed. */
int fmx_top_lines_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                              const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                              const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint8_t *descending, int32_t frac_digits,
                              int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc, int32_t *lines,
                              int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                              int32_t *term_status);
/* ... with class patterns as value patterns and as terms, as fmx_number_stats_where_class_batch; a position is one character of
 * the pattern's length */
int fmx_top_lines_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                    int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off,
                                    int32_t n_terms, int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                    const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint8_t *descending, int32_t frac_digits,
                                    int32_t first, int32_t top, int32_t *rows, int32_t *row_line, int64_t *row_value, int32_t *row_loc,
                                    int32_t *lines, int32_t *numbers, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept,
                                    int32_t *status, int32_t *term_status);

/* STATISTICS BY KEY: THE NUMBER BEHIND A PATTERN, GROUPED BY THE VALUE OF A FIELD OF THE SAME LINE (stats count, sum(bytes=),
 * p95(latency_ms=) by status=) — the host form of the three stages fmx_first_hits_of_lines_dev, fmx_values_of_hits_groups_dev and
 * fmx_numbers_by_key_dev (below).  A call has m KEY PATTERNS (key_pat, key_off) and n NUMBER PATTERNS (pat, pat_off); by_of[i] in
 * [0, m) names the key pattern number pattern i is grouped by, several may share one.  The terms, query_off, term_kind, q and the
 * window of lines [line_lo, line_hi) (0 .. INT32_MAX: every line) are fmx_field_values_where_batch's and its keep rule holds for
 * the key patterns' hits (key_where_of, m ints, each -1 .. q - 1) and for the number patterns' hits (where_of, n ints) alike.
 * THE KEY OF A LINE for key pattern k: among the KEPT hits of k whose line is L (a hit belongs to the line of its first character)
 * the one with the smallest text position; the key is fmx_field_values_batch's VALUE of that hit under stop / n_stop / max_len (its
 * window, cut at the first code unit of the stop set; the empty string is a key; without '\n' in the stop set the window may run
 * into the next line).  A line with no kept hit of k has no key.
 * THE GROUPS of key pattern k are the distinct keys of its lines in fmx_field_values_batch's order, val_off[k] .. val_off[k + 1] of
 * (*lines)[g] = the number of lines that have that key (count of "stats ... by"), (*text_off)[g] .. (*text_off)[g + 1] of *chars
 * its code units; val_off (m + 1 int64, out), val_off[m] = G.  A group may have lines > 0 and no number hit.
 * THE ROWS are packed: row_off (n + 1 int64, out), row_off[i + 1] - row_off[i] = the groups of key by_of[i]; row (i, g) at
 * row_off[i] + g is over the kept hits of number pattern i whose line has key g and that parse (the value of a hit:
 * fmx_number_stats_where_batch): (*count), (*sum_lo), (*sum_hi), (*min), (*max), (*pct)[row * P + j] as there.  Per number pattern:
 * no_key[i] = the kept hits on a line without a key — decided before parsing, such a hit is counted here and nowhere else;
 * not_number[i], overflow[i] = the kept hits on a line with a key that did not parse.  For every i
 *     sum over g of count[row_off[i] + g] + no_key[i] + not_number[i] + overflow[i] = kept[i].
 * occurrences, kept, status (n ints) are the number patterns', key_occurrences, key_kept, key_status (m ints) the key patterns',
 * term_status the terms'; each nullable.  *lines, *text_off, *chars, *count, *sum_lo, *sum_hi, *min, *max and *pct point into ONE
 * allocation owned by the library until fmx_free_buffer((uint8_t *)*lines); all are NULL when there is no group (and on every
 * failure).  When the key patterns have no kept hit nothing beyond the filter runs on the device, there are no groups and no rows
 * and no_key[i] = kept[i]; when the number patterns have none, the groups are reported with zero rows.  On an index built without
 * extraction there are no groups, no rows, every counter is zero and every status is FMX_ST_NOT_ENABLED; occurrences and kept are
 * still filled.  The line table is always required (keys are per line).
 * Two waits beyond the filter's own: the kept offsets (they size the stages) and the m + 1 group offsets (they size the rows), and
 * one for the size of the groups' text.  Scratch: about 30 bytes per kept key hit for stage a, fmx_values_of_hits_groups_scratch_bytes
 * per first hit, fmx_numbers_by_key_scratch_bytes per kept slot.
 * n == 0: FMX_OK, nothing is searched, val_off and row_off are zeroed, term_status is zeroed.  m == 0 with n > 0: FMX_E_ARG.
 * FMX_E_ARG as fmx_field_values_where_batch (max_len outside [1, 64], more than 64 stop units, the query arrays, a where_of or
 * key_where_of outside -1 .. q - 1, a window that is not 0 <= line_lo <= line_hi, kept hits * max_len above 2^35) and as
 * fmx_number_stats_where_batch (frac_digits, n_permille, a permille), for a by_of outside [0, m), more than 2^27 rows or rows *
 * max(P, 1) above 2^27, an index without a line table (the fmx_line_table_build message), a SuffixArray / RrrVector / stand-alone
 * wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing behind. */
int fmx_number_stats_by_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                              const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_pat, const int32_t *term_off,
                              int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *key_where_of,
                              const int32_t *where_of, int32_t line_lo, int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                              int32_t frac_digits, const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines,
                              int64_t **text_off, uint16_t **chars, int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi,
                              int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow,
                              int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept,
                              int32_t *key_status, int32_t *term_status);
/* ... with class patterns as key patterns (key_alt, key_pos_off, key_n_pos, key_off), as number patterns and as terms, each batch as
 * fmx_field_values_where_class_batch takes its own; a position is one character of a pattern's length, so the windows behind a key
 * and behind a number start behind the last position.  The values and numbers behind ALL spellings of a pattern make one answer.
 * key_pos_off and key_off are required even with m == 0.  FMX_E_ARG also as fmx_field_values_where_class_batch judges a class
 * batch (max_ranges outside [1, FMX_CLASS_RANGES_MAX], offsets that decrease, pattern offsets behind the positions) */
int fmx_number_stats_by_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                    const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                    const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_alt, const int32_t *term_pos_off,
                                    int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                    const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                    int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits,
                                    const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off,
                                    uint16_t **chars, int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min,
                                    int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences,
                                    int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status,
                                    int32_t *term_status);

/* STATISTICS BY TWO KEYS: THE NUMBER BEHIND A PATTERN, AND THE LINES, GROUPED BY THE VALUES OF TWO FIELDS OF THE SAME LINE (stats
 * p95(latency_ms=) by host=, status=; the pivot table count by host=, status=) — the host form of stages a and b of STATISTICS BY
 * KEY, fmx_pairs_of_first_hits_dev and fmx_numbers_by_key_dev (below).  The arguments are fmx_number_stats_by_batch's — the m key
 * patterns, the n number patterns, the terms, query_off, term_kind, q, key_where_of, where_of, the window of lines, stop / n_stop /
 * max_len, frac_digits, permille / n_permille — plus n_pairs = c PAIRS pair_a[j], pair_b[j], each in [0, m) and the two may be
 * equal; by_of[i] in [0, c) names the PAIR number pattern i is grouped by.
 * THE GROUPS of the key patterns — val_off, *lines, *text_off, *chars — are fmx_number_stats_by_batch's, so a pair is printed as two
 * values.  Line L has a PAIR KEY for pair j iff it has a key for pair_a[j] and one for pair_b[j]: (ga, gb), the two groups' indexes
 * among their key patterns' groups.  THE PAIRS of j are the distinct (ga, gb) of its lines, ascending by ga, then gb: pair_off (c + 1
 * int64, out), entry r of pair j at pair_off[j] + r of (*pair_group_a), (*pair_group_b) and (*pair_lines) = the lines that have it
 * (at least 1).  The lines of j's pairs add up to the lines with both keys; a pair (k, k) has the pairs (g, g) with pair_lines =
 * lines.
 * THE ROWS are packed: row_off (n + 1 int64, out), row_off[i + 1] - row_off[i] = the pairs of by_of[i]; row (i, r) at row_off[i] + r
 * is over the kept hits of number pattern i whose line has pair r and that parse: (*count) .. (*pct) as fmx_number_stats_by_batch.
 * no_key[i] = the kept hits of i on a line without a pair key, decided before parsing and counted there and nowhere else;
 * not_number[i], overflow[i] as there.  For every i
 *     sum over r of count[row_off[i] + r] + no_key[i] + not_number[i] + overflow[i] = kept[i].
 * occurrences .. term_status as fmx_number_stats_by_batch.  *lines, *text_off, *chars, *pair_group_a, *pair_group_b, *pair_lines,
 * *count .. *pct point into ONE allocation owned by the library until fmx_free_buffer((uint8_t *)*lines); all are NULL when there is
 * no group (and on every failure).
 * n == 0 IS A REAL CALL: the groups, the pairs and their lines (count by a, b); no number stage runs.  m == 0 (then n_pairs and n
 * must be 0): FMX_OK, nothing is searched.  No kept key hit: no groups, no pairs, no_key[i] = kept[i].  No pair at all: the groups
 * are reported, no rows, no_key[i] = kept[i].  No kept number hit: the pairs with zero rows.  An index without extraction: as
 * fmx_number_stats_by_batch (FMX_ST_NOT_ENABLED).  The line table is always required.
 * The waits are fmx_number_stats_by_batch's and ONE more 8 * (c + 1)-byte read of the pair offsets, which sizes the rows.
 * FMX_E_ARG as fmx_number_stats_by_batch, with the pairs in the place of the key patterns for by_of and the rows' limits, and for a
 * pair_a / pair_b outside [0, m), n_pairs > 0 with m == 0, n > 0 with n_pairs == 0, more than 2^31 - 1 kept hits of the a-sides,
 * fm_bits(c) + fm_bits(the most groups of an a-side) + fm_bits(the most groups of a b-side) > 64 (fm_bits(v): the bits of v, at
 * least 1). */
int fmx_number_stats_by_pair_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                                   const int32_t *pat_off, int32_t n, const int32_t *by_of, int32_t n_pairs, const int32_t *pair_a,
                                   const int32_t *pair_b, const uint16_t *term_pat, const int32_t *term_off, int32_t n_terms, const int32_t *query_off,
                                   const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                   int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille,
                                   int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off, uint16_t **chars, int64_t *pair_off,
                                   int32_t **pair_group_a, int32_t **pair_group_b, int32_t **pair_lines, int64_t *row_off, int32_t **count,
                                   uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key,
                                   int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                   int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status);
/* ... with class patterns as key patterns, as number patterns and as terms, each batch as fmx_number_stats_by_class_batch takes its
 * own; its refusals of a class batch */
int fmx_number_stats_by_pair_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                         const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                         const int32_t *pat_off, int32_t n, const int32_t *by_of, int32_t n_pairs, const int32_t *pair_a,
                                         const int32_t *pair_b, const uint16_t *term_alt, const int32_t *term_pos_off, int32_t term_n_pos,
                                         const int32_t *term_off, int32_t n_terms, int32_t max_ranges, const int32_t *query_off,
                                         const uint8_t *term_kind, int32_t q, const int32_t *key_where_of, const int32_t *where_of, int32_t line_lo,
                                         int32_t line_hi, const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits,
                                         const int32_t *permille, int32_t n_permille, int64_t *val_off, int32_t **lines, int64_t **text_off,
                                         uint16_t **chars, int64_t *pair_off, int32_t **pair_group_a, int32_t **pair_group_b, int32_t **pair_lines,
                                         int64_t *row_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max,
                                         int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept,
                                         int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status);

/* STATISTICS BY KEY PER BUCKET: THE NUMBER BEHIND A PATTERN, BY THE VALUE OF A FIELD OF THE SAME LINE, PER BUCKET OF LINES (timechart
 * p95(latency_ms=) by status=: the top few values, each with its statistics per bucket, plus "other") — the host form of stages a
 * and b of STATISTICS BY KEY and fmx_numbers_by_key_buckets_dev (below).  The arguments are fmx_number_stats_by_batch's, word for
 * word — the m key patterns, the n number patterns with by_of, the terms, query_off, term_kind, q, key_where_of, where_of, stop /
 * n_stop / max_len, frac_digits, permille / n_permille — except that edges / n_edges (fmx_number_stats_where_batch's: edges == NULL
 * with n_edges == 0 means B = 1, every line) stand in the place of line_lo / line_hi, and top in [1, 65536] is added.
 * THE HITS OF THE CALL: with edges the filter's window of lines is [edges[0], edges[B]) for key hits and number hits alike, so
 * every kept hit has a bucket.  The line table is always required (keys are per line).
 * THE GROUPS of key pattern k are fmx_number_stats_by_batch's for that window: the distinct keys of its lines in
 * fmx_field_values_batch's order, each with its lines; n_groups[k] = G_k (m ints, out, nullable).  The groups do not come down.
 * THE KEY ROWS of k are its R_k = min(top, G_k) groups with the most lines, in descending order; equal lines stay in value order
 * (the smaller group index first).  key_row_off (m + 1 int64, out, key_row_off[0] = 0) packs them.  Per key row r:
 * (*key_row_lines)[r]; (*key_row_group)[r] = the group's index among the pattern's groups; (*text_off)[r] .. (*text_off)[r + 1] of
 * *chars its code units (key_row_off[m] + 1 int64).
 * THE CELLS of number pattern i with k = by_of[i] number (R_k + 1) * B, packed at cell_off[i] (n + 1 int64, out): cell (i, r, b) at
 * cell_off[i] + r * B + b.  Rows r < R_k are over the kept hits of i that parse and whose line has the key of key row r of k; row
 * r = R_k is "other": the key of the line is a group that is no key row.  Each cell holds (*count), (*sum_lo), (*sum_hi), (*min),
 * (*max) and (*pct)[cell * P + j] exactly as fmx_number_stats_where_batch defines them; an empty cell is all zeros.
 * Per number pattern no_key[i], not_number[i] and overflow[i] are fmx_number_stats_by_batch's (no_key is decided before parsing);
 * occurrences, kept, status, key_occurrences, key_kept, key_status and term_status as there.  For every i
 *     sum over the cells of i of count + no_key[i] + not_number[i] + overflow[i] = kept[i];
 * with top >= G_k and no edges the rows of i, put back in key_row_group order, are fmx_number_stats_by_batch's rows and "other" is
 * zero; with edges, a row's cells summed over b are that call's row for lines = [edges[0], edges[B]); for every (i, b) the cells'
 * counts over all rows plus the hits of bucket b among no_key, not_number and overflow are fmx_hit_histogram_where_batch's counter.
 * *key_row_lines, *key_row_group, *text_off, *chars, *count, *sum_lo, *sum_hi, *min, *max and *pct point into ONE allocation owned
 * by the library until fmx_free_buffer((uint8_t *)*key_row_lines).  When no key pattern has a kept hit nothing beyond the filter
 * runs, all of them are NULL, key_row_off and cell_off are zeroed and no_key[i] = kept[i]; when the number patterns have no kept
 * hit the key rows are reported and every cell is zero.  n == 0, m == 0 with n > 0, an index without extraction, a handle that is
 * not resident and the wrong kind of handle: as fmx_number_stats_by_batch.
 * Only (top + 1) * B cells per number pattern and the text of top keys per key pattern come down, whatever G_k is.  The waits are
 * fmx_number_stats_by_batch's (the kept offsets; the m + 1 group offsets with the size of the groups' text behind them) and the 8
 * bytes of the key rows' packed text length.
 * FMX_E_ARG, judged from the arguments alone and before any device work: everything fmx_number_stats_by_batch refuses, edges as
 * fmx_number_stats_where_batch judges them, top outside [1, 65536], (int64) n * (top + 1) * B above 2^27 or that times max(P, 1)
 * above 2^27.  A refused call stores nothing. */
int fmx_number_stats_by_histogram_batch(const fmx_index *idx, const uint16_t *key_pat, const int32_t *key_off, int32_t m, const uint16_t *pat,
                                        const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_pat, const int32_t *term_off,
                                        int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *key_where_of,
                                        const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop,
                                        int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille, int32_t n_permille,
                                        int32_t *n_groups, int64_t *key_row_off, int32_t **key_row_lines, int32_t **key_row_group, int64_t **text_off,
                                        uint16_t **chars, int64_t *cell_off, int32_t **count, uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min,
                                        int64_t **max, int64_t **pct, int32_t *no_key, int32_t *not_number, int32_t *overflow, int32_t *occurrences,
                                        int32_t *kept, int32_t *status, int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status,
                                        int32_t *term_status);
/* ... with class patterns as key patterns, as number patterns and as terms, each batch as fmx_number_stats_by_class_batch takes its
 * own.  The values and numbers behind ALL spellings of a pattern make one answer. */
int fmx_number_stats_by_histogram_class_batch(const fmx_index *idx, const uint16_t *key_alt, const int32_t *key_pos_off, int32_t key_n_pos,
                                              const int32_t *key_off, int32_t m, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                              const int32_t *pat_off, int32_t n, const int32_t *by_of, const uint16_t *term_alt,
                                              const int32_t *term_pos_off, int32_t term_n_pos, const int32_t *term_off, int32_t n_terms,
                                              int32_t max_ranges, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                              const int32_t *key_where_of, const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top,
                                              const uint16_t *stop, int32_t n_stop, int32_t max_len, int32_t frac_digits, const int32_t *permille,
                                              int32_t n_permille, int32_t *n_groups, int64_t *key_row_off, int32_t **key_row_lines,
                                              int32_t **key_row_group, int64_t **text_off, uint16_t **chars, int64_t *cell_off, int32_t **count,
                                              uint64_t **sum_lo, uint64_t **sum_hi, int64_t **min, int64_t **max, int64_t **pct, int32_t *no_key,
                                              int32_t *not_number, int32_t *overflow, int32_t *occurrences, int32_t *kept, int32_t *status,
                                              int32_t *key_occurrences, int32_t *key_kept, int32_t *key_status, int32_t *term_status);

/* TOP VALUES PER BUCKET: THE TOP VALUES OF A FIELD PER BUCKET OF LINES, the stacked timeline (count by status over time where line
 * has user=svc3: the ten most frequent values, each with its counts per bucket, plus "other") — the host forms of
 * fmx_values_of_hits_groups_dev, fmx_values_top_histogram_dev and fmx_values_gather_rows_dev (below: the stages).  The value
 * patterns, terms, query_off, term_kind, q, where_of, stop, n_stop and max_len are fmx_field_values_where_batch's, and so are a hit's
 * value and the order of values; edges and n_edges are fmx_number_stats_where_batch's: edges == NULL with n_edges == 0 means B = 1,
 * every line (no line table is needed unless a pattern asks for a query), otherwise the edge rules above.  top lies in [1, 65536].
 * THE HITS OF THE CALL: with edges the filter's window of lines is [edges[0], edges[B]), so every kept hit has a bucket; kept[i] is
 * the number of those hits, occurrences[i] stays the count in the whole text.  The values stage runs over the kept hits only.
 * THE GROUPS of pattern i are fmx_field_values_where_batch's values and counts for that window, n_values[i] = G_i of them (n ints,
 * out, nullable).
 * THE ROWS of pattern i are its R_i = min(top, G_i) groups with the largest counts, in descending order of count; equal counts stay
 * in value order (the smaller group index first).  row_off (n + 1 int64, out, row_off[0] = 0) packs them, R = row_off[n].  Per row
 * r: (*row_count)[r] = the kept hits that have the value; (*row_group)[r] = the value's index among the pattern's distinct values in
 * value order; (*text_off)[r] .. (*text_off)[r + 1] of *chars its code units (R + 1 int64); (*hist)[r * B + b] = the hits of that
 * value in bucket b.  other (the caller's n * B ints): other[i * B + b] = the kept hits of pattern i in bucket b whose value is no
 * row.  For every row the sum over b of hist[r * B + b] is row_count[r]; for every i and b the rows' hist[., b] and other[i * B + b]
 * add up to hist[i * B + b] of fmx_hit_histogram_where_batch for the same call (with edges == NULL: to kept[i]); with top >= G_i
 * the rows of i, sorted back by row_group, are fmx_field_values_where_batch's values and counts and other is zero.
 * *row_count, *row_group, *text_off, *chars and *hist point into ONE allocation owned by the library until
 * fmx_free_buffer((uint8_t *)*row_count); all are NULL when R = 0 (and on every failure).  On an index built without extraction
 * every status is FMX_ST_NOT_ENABLED, there are no rows and other is zero; occurrences and kept are still filled.
 * FMX_ST_TOO_MANY_RANGES (class form) as in fmx_field_values_where_class_batch.
 * Only top * B counters and the text of top values per pattern come down, whatever G_i is.  Three waits beyond the filter's own: the
 * kept offsets (they size the stages), ONE read of the n + 1 group offsets with the size of the groups' text behind them, and the 8
 * bytes of the rows' packed text length.  Scratch: fmx_values_of_hits_groups_scratch_bytes and
 * fmx_values_top_histogram_scratch_bytes per kept hit, four bytes per code unit of the groups' text.
 * n == 0: FMX_OK, nothing is searched, row_off[0] = 0, term_status is zeroed.
 * FMX_E_ARG as fmx_field_values_where_batch (max_len outside [1, 64], more than 64 stop units, the query arrays, a where_of outside
 * -1 .. q - 1, kept hits * max_len above 2^35) and as fmx_number_stats_where_batch judges edges (an index without a line table:
 * only when edges are given or a pattern asks for a query), for top outside [1, 65536] and for (int64) n * (top + 1) * B above
 * 2^27; FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_NOMEM leaves nothing behind.  A refused call stores nothing. */
int fmx_field_values_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                           const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                           const int32_t *where_of, const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop,
                                           int32_t n_stop, int32_t max_len, int32_t *n_values, int64_t *row_off, int32_t **row_count,
                                           int32_t **row_group, int64_t **text_off, uint16_t **chars, int32_t **hist, int32_t *other,
                                           int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status);
/* ... with class patterns as value patterns and as terms, as fmx_field_values_where_class_batch; a position is one character of the
 * pattern's length.  The values behind ALL spellings of a pattern make one answer. */
int fmx_field_values_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                                 const int32_t *pat_off, int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off,
                                                 int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                                                 const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *where_of,
                                                 const int32_t *edges, int32_t n_edges, int32_t top, const uint16_t *stop, int32_t n_stop,
                                                 int32_t max_len, int32_t *n_values, int64_t *row_off, int32_t **row_count, int32_t **row_group,
                                                 int64_t **text_off, uint16_t **chars, int32_t **hist, int32_t *other, int32_t *occurrences,
                                                 int32_t *kept, int32_t *status, int32_t *term_status);

/* DISTINCT VALUES PER BUCKET: THE NUMBER OF DIFFERENT VALUES OF A FIELD PER BUCKET OF LINES (timechart dc(user=); countDistinct,
 * cardinality) and, beside it, THE VALUES SEEN FOR THE FIRST TIME in each bucket (new block ids, new error classes, new users per
 * minute) — the host forms of fmx_values_of_hits_groups_dev and fmx_values_distinct_histogram_dev (below: the stage).  The arguments
 * are fmx_field_values_histogram_where_batch's without top: the value patterns, terms, query_off, term_kind, q, where_of, stop,
 * n_stop and max_len, and edges with n_edges (edges == NULL with n_edges == 0 means B = 1, every line; no line table is needed then
 * unless a pattern asks for a query).  THE HITS OF THE CALL: with edges the filter's window of lines is [edges[0], edges[B]), so
 * every kept hit has a bucket.  The value of a hit is fmx_field_values_batch's, exactly; a hit belongs to the line of its first
 * character; the buckets follow the edge rules above.  Per pattern i:
 *   distinct[i * B + b]    the number of different values among the kept hits of i in bucket b;
 *   first_seen[i * B + b]  the number of values of i whose FIRST kept hit — the one with the smallest line, and therefore the
 *                          smallest bucket — lies in bucket b;
 *   n_values[i] (nullable), occurrences[i], kept[i], status[i] and term_status[t] as in fmx_field_values_histogram_where_batch.
 * distinct and first_seen are the caller's n * B ints each: nothing is allocated, nothing is to be freed.  It follows that the sum
 * over b of first_seen[i, b] is n_values[i]; first_seen <= distinct <= fmx_hit_histogram_where_batch's counter, elementwise, and
 * distinct is 0 exactly where that counter is; max_b distinct[i, b] <= n_values[i] <= the sum over b of distinct[i, b]; without
 * edges distinct[i] == first_seen[i] == n_values[i]; and distinct[i, b] is the number of rows of
 * fmx_field_values_histogram_where_batch with top >= G_i whose hist[r, b] is positive.
 * n * B pairs of ints come down, whatever the number of values is, and no value's text is filled.  Two waits beyond the filter's
 * own: the kept offsets (they size the stages) and ONE read of the n + 1 group offsets.  Scratch:
 * fmx_values_of_hits_groups_scratch_bytes and fmx_values_distinct_histogram_scratch_bytes per kept hit.  On an index built without
 * extraction every status is FMX_ST_NOT_ENABLED and every counter is zero; occurrences and kept are still filled.
 * FMX_ST_TOO_MANY_RANGES (class form) as in fmx_field_values_where_class_batch.  n == 0: FMX_OK, nothing is searched, term_status
 * is zeroed.  FMX_E_ARG as fmx_field_values_histogram_where_batch (an index without a line table — see fmx_line_table_build — only
 * when edges are given or a pattern asks for a query) and for (int64) n * B above 2^27; FMX_E_NO_DEVICE for a handle that is not
 * resident.  A refused call stores nothing. */
int fmx_distinct_values_histogram_where_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const uint16_t *term_pat,
                                              const int32_t *term_off, int32_t n_terms, const int32_t *query_off, const uint8_t *term_kind,
                                              int32_t q, const int32_t *where_of, const int32_t *edges, int32_t n_edges, const uint16_t *stop,
                                              int32_t n_stop, int32_t max_len, int32_t *distinct, int32_t *first_seen, int32_t *n_values,
                                              int32_t *occurrences, int32_t *kept, int32_t *status, int32_t *term_status);
/* ... with class patterns as value patterns and as terms, as fmx_field_values_where_class_batch; a position is one character of the
 * pattern's length.  The values behind ALL spellings of a pattern make one answer. */
int fmx_distinct_values_histogram_where_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos,
                                                    const int32_t *pat_off, int32_t n, const uint16_t *term_alt, const int32_t *term_pos_off,
                                                    int32_t term_n_pos, const int32_t *term_off, int32_t n_terms, int32_t max_ranges,
                                                    const int32_t *query_off, const uint8_t *term_kind, int32_t q, const int32_t *where_of,
                                                    const int32_t *edges, int32_t n_edges, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                                                    int32_t *distinct, int32_t *first_seen, int32_t *n_values, int32_t *occurrences, int32_t *kept,
                                                    int32_t *status, int32_t *term_status);

/* THE LINES THAT MATCH A QUERY WITH TERMS ON NUMBERS (latency_ms >= 500; size in 0 .. 67108863; status in 500 .. 599) — the host
 * forms of the two packed stages + fmx_hits_in_number_range_dev (below: the stage) + fmx_query_lines_of_hits_dev.  They are
 * fmx_match_query_batch's calls and its definitions hold unchanged: the n TERMS, query_off, term_kind (ALL / ANY / NONE; a query of
 * NONE terms only has no lines), q, max_lines, line_off, *lines (the ONE allocation, freed with fmx_free_buffer), line_count,
 * occurrences and status.  The one addition: num_lo and num_hi (n int64 each, host) and ONE frac_digits F in [0, 9].
 * Term t is RANGED iff num_lo[t] >= 0 (a value is never negative: a negative num_lo[t] is a plain string term).  A hit of a ranged
 * term has THE VALUE OF A HIT of fmx_number_stats_where_batch above, exactly (the window of 32 code units behind the term, F as
 * there), and PASSES iff it parses and num_lo[t] <= value <= num_hi[t]; "not a number" and "overflow" never pass, whatever num_hi
 * is (a run of 32 digits and a value above 2^63 - 1 included).  num_hi[t] = INT64_MAX is "no upper bound"; num_lo[t] > num_hi[t]
 * is legal and keeps nothing.  The filter runs over the located hits between the fill and the line stage: a ranged term HOLDS on a
 * line iff one of its PASSING hits lies there.  So the NONE term ("size ", 67108864, INT64_MAX) removes the lines whose size is at
 * least 64 MiB, and lines whose "size " is not a number stay.
 * occurrences[t] stays count() in the whole text.  kept[t], not_number[t], overflow[t] (each nullable, n ints): the hits of term t
 * that pass, and those that did not parse, by reason — an unranged term: every hit, 0, 0 —, so
 *     kept[t] + not_number[t] + overflow[t] <= occurrences[t],   the rest are numbers outside the range;
 * with num_lo[t] = 0 and num_hi[t] = INT64_MAX the three are count, not_number and overflow of fmx_number_stats_where_batch for
 * that pattern without edges and without a filter.  A window the packed extract ran literally hands its status to its term.  On
 * an index built without extraction every ranged term gets FMX_ST_NOT_ENABLED and keeps no hit; unranged terms are unaffected.
 * num_lo == NULL && num_hi == NULL: the answer is, array for array, fmx_match_query_batch's (kept = the occurrences), and an index
 * without extraction still answers; one of them NULL alone is FMX_E_ARG.
 * Device scratch: fmx_match_query_batch's, with fmx_hits_in_number_range_scratch_bytes (about 130 bytes per hit of the batch) in
 * front and the line stage's 40 bytes per KEPT hit: ONE 8-byte read and wait brings the kept total down and sizes the line stage,
 * one more the number of lines.  What comes down is the lines and the small per-term arrays — the hits and their text do not.
 * Errors as fmx_match_query_batch, and FMX_E_ARG for frac_digits outside [0, 9]. */
int fmx_match_query_number_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, const int64_t *num_lo,
                                 const int64_t *num_hi, int32_t frac_digits, const int32_t *query_off, const uint8_t *term_kind, int32_t q,
                                 int32_t max_lines, int64_t *line_off, int32_t **lines, int32_t *line_count, int32_t *occurrences, int32_t *kept,
                                 int32_t *not_number, int32_t *overflow, int32_t *status);
/* ... with class patterns as terms, as fmx_match_query_class_batch; a position is one character of the pattern's length */
int fmx_match_query_number_class_batch(const fmx_index *idx, const uint16_t *alt, const int32_t *pos_off, int32_t n_pos, const int32_t *pat_off,
                                       int32_t n, int32_t max_ranges, const int64_t *num_lo, const int64_t *num_hi, int32_t frac_digits,
                                       const int32_t *query_off, const uint8_t *term_kind, int32_t q, int32_t max_lines, int64_t *line_off,
                                       int32_t **lines, int32_t *line_count, int32_t *occurrences, int32_t *kept, int32_t *not_number,
                                       int32_t *overflow, int32_t *status);

/* THE TEXT OF RANGES AND LINES IN ONE PACKED ARRAY (extract, FM:564-608, batched) — the host form of
 * fmx_extract_packed_offsets_dev + fmx_extract_packed_fill_dev (below: the layout, the statuses, how the work is cut).
 * host buffers, synchronous: text_off = n + 1 int64 (out), text_off[0] = 0; *chars = text_off[n] UTF-16 code units owned by the
 * library until fmx_free_buffer((uint8_t *)*chars) (NULL when there are none, and on every failure); status nullable, n ints.
 * (*chars)[text_off[i] .. text_off[i + 1]) is what extract(start[i], stop[i], destination, 0) leaves in destination[0 .. stop -
 * start).  Memory follows the SUM of the lengths, not n times the longest.  One index on one device and one device buffer for
 * the whole answer in this version: FMX_E_NOMEM when it, or the result, cannot be allocated (nothing is left behind);
 * FMX_E_ARG for null or negative arguments, for an answer of more than 2^35 characters, and for a SuffixArray, RrrVector or
 * stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident.  n == 0: FMX_OK, text_off[0] = 0. */
int fmx_extract_packed_batch(const fmx_index *idx, const int32_t *start, const int32_t *stop, int32_t n, int64_t *text_off,
                             uint16_t **chars, int32_t *status);
/* ... of LINES: the ids go through the resident line table on the device (fmx_line_table_build; fmx_line_bounds_batch's rule)
 * and nothing in between comes down.  An id that is no line gets FMX_ST_POS_NEGATIVE and length 0.  FMX_E_ARG without a table. */
int fmx_line_text_batch(const fmx_index *idx, const int32_t *lines, int32_t n, int64_t *text_off, uint16_t **chars, int32_t *status);
/* how many ranges the calling thread's last fmx_extract_packed_batch / fmx_line_text_batch — or windows its last
 * fmx_field_values_batch / fmx_field_values_class_batch or their _where forms — ran literally (the redo list below); -1 before the first such call.  0 on
 * an index without quirk rows. */
int64_t fmx_extract_packed_last_redo(void);

/* int extract(int start, int stop, char[] destination, int offset) FM:564-608.  dst is n rows of
 * dst_len chars (row i = the `destination` array of query i, in/out); out_len[i] = return value. */
int fmx_extract_batch(const fmx_index *idx, const int32_t *start, const int32_t *stop, int32_t n, uint16_t *dst,
                      int32_t dst_len, int32_t offset, int32_t *out_len, int32_t *lf_steps, int32_t *status);

/* extractUntilBoundary FM:640-759 (mode 0), extractUntilBoundaryLeft FM:772-831 (mode 1),
 * extractUntilBoundaryRight FM:844-922 (mode 2).  aux[i] = N of "Currently extracted: N". */
int fmx_extract_boundary_batch(const fmx_index *idx, const int32_t *from, int32_t n, uint16_t boundary, int mode,
                               uint16_t *dst, int32_t dst_len, int32_t offset, int32_t *out_len,
                               int32_t *lf_steps, int32_t *status, int32_t *aux);

/* ---- batched queries: device-resident buffers, asynchronous on `stream` (a hipStream_t) ----
 * Same semantics; every pointer is device memory on the index's device.  Nothing is synchronised:
 * the caller orders work through the stream (this is what bench.py times with HIP events).
 * Threading: the index is immutable once resident (the reference's FmIndex is @ThreadSafe, FM:82).  The host-buffer
 * entry points above may be called from any number of threads on one index at once (per-call device scratch).
 * The device-pointer entry points keep grow-only scratch per (index, stream): use one stream per thread. */
int fmx_count_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                        int32_t *d_counts, int32_t *d_lf_steps, int32_t *d_status, void *stream);
/* The two stages of fmx_count_batch_dev, callable separately (bench.py times the second one alone):
 * plan = processing order of the batch (device bucket pass on the patterns' trailing characters, so that
 * neighbouring lanes walk the same SA intervals) + the mapped codes of each pattern's last characters; *d_plan is
 * an opaque handle into per-stream scratch owned by the index, or NULL for small batches.  It stays valid until
 * ANYTHING else plans on that stream (every count / locate / segment / pipeline call does) and only for the same
 * d_pat / d_pat_off contents.  ordered = the k_count kernel over that order; a handle that is no longer the
 * stream's live plan — or that was made for other d_pat / d_pat_off BUFFERS or another n — is ignored (the batch is
 * then processed in the caller's order: same results).  The library compares buffer addresses, not contents: a
 * caller that refills d_pat or d_pat_off in place must plan again.  Results are written at the ORIGINAL pattern index. */
int fmx_count_plan_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                       const void **d_plan, void *stream);
int fmx_count_ordered_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, const void *d_plan,
                          int32_t n, int32_t *d_counts, int32_t *d_lf_steps, int32_t *d_status, void *stream);
/* 1 if fmx_count_batch_dev / fmx_locate_batch_dev would run the plan stage for a batch of n patterns on this resident index, 0 if
 * they count in the caller's order — results are the same either way.  On an index with a suffix table the plan orders the
 * batch by the (estimated) first SA row of each pattern's tabulated suffix (option "plan_sa_key": 2 = estimated from the table's
 * two-character strings, the default; 1 = the table's own answer; 0 = by the trailing characters' codes, as on an index
 * without a table) and pays from "plan_sa_min" patterns on (option, default 786,432); with "plan_sa_key" 0 a batch is planned
 * if it holds at least "plan_min_per_string" (default 16) patterns per string of the table's deepest level.  An index without a
 * table plans every batch of "sort_min" patterns or more.  (fmx_count_plan_dev always plans: the caller asked.)
 * locate has an order of its own on top: batches of "walk_order_min" patterns or more (default 32,768; 0 = never) walk their
 * hits by the first row of the patterns' SA ranges ("walk_fine" = 0 drops that order's fine pass); extractUntilBoundary batches
 * of "boundary_order_min" queries or more (default 32,768) are taken by text position.  No order changes a result. */
int fmx_count_batch_is_planned(const fmx_index *idx, int32_t n);
/* The same question for every batch policy: kind 0 = count() planned (as above), 1 = locate() walks its hits by the first row
 * of the patterns' SA ranges ("walk_order_min"), 2 = extractUntilBoundary takes its queries by text position
 * ("boundary_order_min").  1 / 0; results never depend on the answer. */
int fmx_batch_policy(const fmx_index *idx, int kind, int64_t n);
int fmx_locate_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                         int32_t max_matches, int32_t *d_locs, int32_t loc_cap, int32_t *d_found,
                         int32_t *d_lf_steps, int32_t *d_status, int32_t *d_range_ws /* 2*n ints */, void *stream);
/* int locate(char[] pattern, int[] locations) FM:487-489 — "all occurrences", the loop of FM:526-548 without a limit (FM:487-552)
 * — for a batch, PACKED: one offsets array of n + 1 entries and one array of positions, so that a batch that mixes patterns of
 * one hit with a pattern of millions takes the memory of its hits (fmx_locate_batch's rows would take n x the largest count), and
 * lanes are handed to HITS, not to patterns: a single pattern with 10^6 hits is spread over the whole device.  Two stages, so
 * that a device caller can allocate d_locs between them:
 * stage 1: the range search of FM:506-523 for the batch, and the packed layout of its hits.
 * d_hit_off[i] = number of hits of patterns 0 .. i-1 (int64; d_hit_off[0] = 0, d_hit_off[n] = all hits of the batch), where
 * pattern i has min(count, max_matches) hits for max_matches > 0 and count hits otherwise (FM:544-546: -1 and 0 never stop).
 * d_lf_steps / d_status (nullable) as fmx_locate_batch_dev's range pass leaves them (an empty pattern: FMX_ST_JAVA_AIOOBE, no hits).
 * d_range_ws = 2*n ints, handed unchanged to stage 2.  Asynchronous on `stream`; nothing is synchronised.
 * n == 0: d_hit_off[0] = 0 (an asynchronous memset).  FMX_E_ARG for null or negative arguments and for a SuffixArray, RrrVector
 * or stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident.  Scratch per (index, stream), like the other
 * device forms.  v1: the patterns are taken in the caller's order after the count plan (no walk-order stage), one index, one
 * device (no segment sets, no *_multi form). */
int fmx_locate_all_ranges_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                              int32_t max_matches, int64_t *d_hit_off, int32_t *d_lf_steps, int32_t *d_status,
                              int32_t *d_range_ws, void *stream);
/* stage 2: hits [first_hit, first_hit + n_hits) of the packed order, cut at d_hit_off[n]: d_locs[t - first_hit] = what the reference's
 * locate() stores for hit t - d_hit_off[p] of its pattern p (SA rows start+1.. in order, FM:527-547).  Entries of d_locs for hits
 * beyond d_hit_off[n] keep the caller's values.  Walk LF-steps are ADDED to d_lf_steps[p], walk statuses OR-ed into d_status[p]
 * (both nullable): windows that tile the hits once give fmx_locate_batch's totals.  d_lf_steps stays int32 per pattern, like
 * fmx_locate_batch's: a pattern whose walks pass 2^31 steps wraps, there as here.  The kernel reads d_hit_off[n] itself (the
 * grid is sized from n_hits): no host synchronisation; d_locs must hold min(n_hits, d_hit_off[n] - first_hit) ints. */
int fmx_locate_all_fill_dev(const fmx_index *idx, int32_t n, const int64_t *d_hit_off, const int32_t *d_range_ws,
                            int64_t first_hit, int64_t n_hits, int32_t *d_locs, int32_t *d_lf_steps, int32_t *d_status,
                            void *stream);
/* EXTRACT, PACKED, in two stages over device pointers; asynchronous on `stream`, nothing is allocated, no host wait.
 * stage 1: d_status[i] = the status FM:566-576 raise for (d_start[i], d_stop[i]), in their order — FMX_ST_NOT_ENABLED,
 * FMX_ST_POS_NEGATIVE, FMX_ST_STOP_TOO_LONG, then FMX_ST_JAVA_AIOOBE for a negative IntVector index (FMX_ST_DEST_TOO_SMALL cannot
 * occur: every range gets the room it needs); d_text_off (n + 1 int64, d_text_off[0] = 0) = the exclusive sum of the lengths: stop
 * - start, and 0 for a range with a status or with stop <= start (which is FMX_ST_OK); d_piece_off (n + 1 int64) = the exclusive
 * sum of the ranges' PIECES.  A range is cut at multiples of P in text coordinates, P = the smallest multiple of the sample rate
 * that is >= 32: every piece but a range's last ends on a position sample, so each is an independent walk of at most P +
 * sampleRate LF-steps for one lane, and a batch is balanced by pieces, not by ranges.  The sums are int64: they do not wrap.
 * The caller reads d_text_off[n] between the stages and gives d_chars that many code units.
 * stage 2: d_chars[d_text_off[i] .. d_text_off[i + 1]) = what extract(start, stop, destination, 0) leaves in destination[0 .. stop
 * - start) — the reference's quirks included: a piece whose walk meets a step that is not clean (a status, or a route through the
 * wavelet tree on which the reference's own result differs from the text) stores no further and puts its RANGE on a redo list,
 * once; a second launch, which reads the list's count on the device, runs the literal extract for those ranges, one lane each,
 * into the same slice and leaves its status in d_status.  On an index without such rows the list stays empty.  Code units of
 * d_chars outside [0, d_text_off[n]) and d_status of the other ranges keep their values.  No per-range LF-steps in this version.
 * scratch: at least *bytes of fmx_extract_packed_scratch_bytes(idx, n, &bytes), the same block for both stages (256-byte aligned); after stage 2 its first int32 is the number of ranges that were redone.
 * FMX_E_ARG for null or negative arguments and a scratch that is too small (nothing is launched); FMX_E_NO_DEVICE for a handle
 * that is not resident.  n == 0: stage 1 zeroes the two offsets' first entry, stage 2 does nothing. */
int fmx_extract_packed_scratch_bytes(const fmx_index *idx, int32_t n, size_t *bytes);
int fmx_extract_packed_offsets_dev(const fmx_index *idx, const int32_t *d_start, const int32_t *d_stop, int32_t n,
                                   int64_t *d_text_off, int64_t *d_piece_off, int32_t *d_status, void *scratch,
                                   size_t scratch_bytes, void *stream);
int fmx_extract_packed_fill_dev(const fmx_index *idx, const int32_t *d_start, const int32_t *d_stop, int32_t n,
                                const int64_t *d_text_off, const int64_t *d_piece_off, uint16_t *d_chars, int32_t *d_status,
                                void *scratch, size_t scratch_bytes, void *stream);
/* THE LINE TABLE of a resident FM-index — a resident extra like the row table and the window directory, 4 bytes per line, made
 * on request: T = the positions locate(new char[]{boundary}, locations) returns, sorted ascending, as int32 in the index's
 * device memory.  It holds what the INDEX answers (quirk Q1 included), not what the text "really" holds, so that everything
 * below is defined by reference calls plus arithmetic:
 *   line(p)  = the number of entries of T below p, for any int32 p;
 *   n_lines  = |T| + 1 if the text is not empty and its last character is not in T, |T| otherwise (the text: what the caller
 *              handed to the constructor, textLength = getInputLength() - 1 characters);
 *   line k   = [k == 0 ? 0 : T[k - 1] + 1, k < |T| ? T[k] : textLength) — the boundary itself excluded;
 *   a hit belongs to the line of its FIRST character, also for a pattern that holds the boundary or is the boundary.
 * Built on the device: the range search and k_locate_all for the one-character pattern, then a device sort.  Host-synchronous.
 * A second call with the same boundary does nothing; another boundary replaces the table.  *n_lines (nullable) = n_lines.
 * The table belongs to the resident state: fmx_free and a new fmx_to_device free it (fmx_line_table_info then reports boundary
 * -1 and 0 bytes), fmx_replicate does not copy it (a replica builds its own).  It is the ONE mutation of a resident index:
 * fmx_line_table_build must not run beside queries on the same handle (every other call on a resident handle may).
 * FMX_E_NO_DEVICE for a handle that is not resident; FMX_E_ARG for a SuffixArray, RrrVector or stand-alone wavelet handle;
 * FMX_E_NOMEM when the table does not fit the device. */
int fmx_line_table_build(fmx_index *idx, uint16_t boundary, int64_t *n_lines);
/* *boundary = the table's boundary character (-1: no table), *n_boundaries = |T|, *bytes = its size as allocated (each nullable) */
int fmx_line_table_info(const fmx_index *idx, int32_t *boundary, int64_t *n_boundaries, int64_t *bytes);
/* fmx_line_bounds_batch over device pointers, asynchronous on `stream` */
int fmx_line_bounds_batch_dev(const fmx_index *idx, const int32_t *d_lines, int32_t n, int32_t *d_start, int32_t *d_stop, void *stream);
/* PACKED HITS -> PACKED DISTINCT LINES.  Input: exactly what fmx_locate_all_ranges_dev and fmx_locate_all_fill_dev leave —
 * d_hit_off (n + 1 entries) and d_locs, which holds hits [0, n_hits) of the packed order, n_hits >= d_hit_off[n] (what the caller
 * read between the stages).  Output: d_line_count[i] (nullable) = the distinct lines of pattern i; d_line_off (n + 1 int64) = the
 * exclusive sum of max_lines > 0 ? min(line_count, max_lines) : line_count; d_lines[d_line_off[i] .. d_line_off[i + 1]) = the
 * distinct line ids of pattern i, ascending (with a limit: the smallest max_lines of them).  The caller gives d_lines room for
 * n_hits ints; entries from d_line_off[n] on keep the caller's values.
 * Lanes are handed to HITS in every stage (a key per hit, ONE device-wide radix sort of (pattern, line) keys, a scan over the
 * sorted keys, a compaction): a batch of one pattern that matches everywhere uses the whole device, and the result does not
 * depend on scheduling (no atomics).  Asynchronous on `stream`; nothing is synchronised and nothing is allocated: the caller
 * owns d_ws, at least fmx_lines_of_hits_scratch_bytes(n, n_hits) bytes (24 per hit — two key arrays, flags, their scan — plus the
 * radix sort's temporary storage, about one more 8-byte key per hit; 0 for an empty call).
 * n == 0 or n_hits == 0: the offsets are zeroed and nothing else is written.  FMX_E_ARG for null or negative arguments, for a
 * workspace that is too small (nothing is launched), without a line table, and for n_hits > 2^31 - 1 in this version;
 * FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits);
int fmx_lines_of_hits_dev(const fmx_index *idx, int32_t n, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                          int32_t max_lines, int64_t *d_line_off, int32_t *d_lines, int32_t *d_line_count, void *d_ws,
                          size_t ws_bytes, void *stream);
/* the grids fmx_lines_of_hits_dev launches for n_hits hits on this index's device: workgroups of the key kernel (a tile of 1,024
 * hits each, per round) and of the element-wise kernels (256 lanes); what is beyond them is taken by grid-stride loops */
int fmx_hit_lines_geometry(const fmx_index *idx, int64_t n_hits, int32_t *key_grid, int32_t *flat_grid);
/* PACKED HITS OF A BATCH OF TERMS -> THE PACKED DISTINCT LINES OF EACH QUERY.  The n patterns of the two packed stages are TERMS;
 * query_off (q + 1 ints: query_off[0] = 0, never decreasing, query_off[q] = n) cuts them into q queries, and term_kind[t] says
 * what term t asks of a line: FMX_TERM_ALL (0) the line must hold it, FMX_TERM_ANY (1) the line must hold at least one of its
 * query's ANY terms (if the query has any), FMX_TERM_NONE (2) the line must not hold it.  With lines(t) = exactly what
 * fmx_lines_of_hits_dev answers for pattern t without a limit (a hit belongs to the line of its first character; the line table
 * is what the index answers), the lines of query Q are
 *     the intersection of lines(t) over Q's ALL terms, intersected with the union of lines(t) over Q's ANY terms if Q has any,
 *     less the union of lines(t) over Q's NONE terms;
 * ascending, every line once.  A query without an ALL and without an ANY term — only NONE terms, or no terms — has NO lines:
 * NONE filters, it does not enumerate the text.  The same pattern may stand twice in a query: two terms.  A term without hits
 * (an empty pattern among them) empties its query as an ALL term and filters nothing as a NONE term.
 * query_off and term_kind are HOST arrays, here too (as seg_base is in the segment forms): the call validates them, derives its
 * tables from them (the query of every term, the ALL and ANY terms of every query) and has copied those into d_ws when it
 * returns — the caller may free or change the arrays at once.  That copy is the one thing the call waits for (a copy from
 * pageable host memory: the runtime has read the source when the call comes back); nothing else is synchronised, nothing is
 * allocated on the device, everything runs on `stream`.
 * Input: exactly what fmx_locate_all_ranges_dev (max_matches = -1) and fmx_locate_all_fill_dev leave — d_hit_off (n + 1 entries)
 * and d_locs, which holds hits [0, n_hits) of the packed order, n_hits >= d_hit_off[n].  Output: d_line_count[Q] (nullable, q
 * entries) = the lines of query Q; d_line_off (q + 1 int64) = the exclusive sum of max_lines > 0 ? min(line_count, max_lines) :
 * line_count; d_lines[d_line_off[Q] .. d_line_off[Q + 1]) = the line ids of query Q, ascending (with a limit: the smallest
 * max_lines of them).  The caller gives d_lines room for n_hits ints (there are never more lines than hits); entries from
 * d_line_off[q] on keep the caller's values.
 * Lanes are handed to hits, to sorted keys or to (query, line) groups in every stage: a key query | line | term per hit, ONE
 * device-wide radix sort, a word per distinct key (an ALL count and two flags), a reduction by (query, line), a scan, a
 * compaction — ONE query whose terms match everywhere uses the whole device, and the result does not depend on scheduling.
 * THE KEY-WIDTH LIMIT: bits(q) + bits(|T|) + bits(the largest number of terms in one query) <= 64, where bits(v) is the number
 * of binary digits of v (1 for 0) and |T| the boundaries of the line table; the per-group word itself sets no smaller limit.
 * d_ws: at least fmx_query_lines_scratch_bytes(n, q, n_hits) bytes (40 per hit — two key arrays, the group heads and their
 * words, 8 each; flags and their scan, 4 each — plus the tables and rocPRIM's temporary storage; 0 for an empty call).
 * q == 0 or n_hits == 0 (n == 0 among them): the q + 1 offsets are zeroed and nothing else is written.  FMX_E_ARG for null or
 * negative arguments, a bad query_off (see above), a kind above 2, a workspace that is too small (nothing is launched, nothing
 * is written), an index without a line table (fmx_last_error names fmx_line_table_build), n_hits > 2^31 - 1, the key-width
 * limit, a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_query_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits);
int fmx_query_lines_of_hits_dev(const fmx_index *idx, int32_t n, int32_t q, const int32_t *query_off, const uint8_t *term_kind,
                                const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int32_t max_lines,
                                int64_t *d_line_off, int32_t *d_lines, int32_t *d_line_count, void *d_ws, size_t ws_bytes,
                                void *stream);
/* A SEQUENCE OF TERMS IN ORDER over device pointers, after the two packed stages of the literal or the class search: (d_hit_off,
 * d_locs) hold the hits of n TERMS; query_off (q + 1 ints, the rule above) cuts them into q SEQUENCES: sequence Q is the terms
 * t_0 .. t_{k-1} = query_off[Q] .. query_off[Q + 1] - 1 IN THAT ORDER; term_len[t] >= 0 is the length of term t.  The hits of a
 * term are exactly what the locate stage reports for it (the reference's answers, quirk rows included).  With [start, stop) the
 * bounds of line L (fmx_line_bounds_batch), L belongs to sequence Q iff there are hits h_0 .. h_{k-1}, h_j a hit of t_j, with
 *     start <= h_0,   h_j + len_j <= h_{j+1} for every j,   h_{k-1} + len_{k-1} <= stop:
 * the occurrences lie inside the line, in order, without overlap — for literals the regular expression t_0.*t_1.* ... on a line.
 * A sequence without terms has no lines; neither has one with a term without hits.  A ONE-TERM sequence is fmx_lines_of_hits_dev
 * of that term LESS the hits that run over the line's end (the boundary pattern itself has no lines here).
 * query_off and term_len are HOST arrays: validated, and copied into d_ws before the call returns.
 * d_line_count (nullable, q entries), d_line_off (q + 1 int64), d_lines: as fmx_query_lines_of_hits_dev, per sequence.  d_spans
 * (nullable, 2 ints per stored line, in the order of d_lines): span_start = the smallest hit of t_0 in the line, span_stop = the
 * end of the chain that takes, term by term, the EARLIEST hit that still fits — what the non-greedy t_0.*?t_1.*? ... matches at
 * its leftmost start: the leftmost start and, from there, the earliest end; NOT the tightest window of the line.
 * That earliest-fit chain from the line's first t_0 hit is also the membership test, and it is exact: any other chain starts
 * later, and every later bound only moves right.  The stages hand lanes to hits (a key term | position per hit, ONE device-wide
 * radix sort — term t's positions then stand ascending in [hit_off[t], hit_off[t + 1]) —, a lane per sorted hit that chains where
 * it opens a line of a first term, a scan, a compaction); integers only, no atomics: the result does not depend on scheduling.
 * d_ws: at least fmx_sequence_lines_scratch_bytes(n, q, n_hits) bytes (36 per hit — two key arrays 8 each, positions, flags,
 * their scan, lines and chain ends 4 each — plus the tables and rocPRIM's temporary storage; 0 for an empty call).  The grids are
 * fmx_hit_lines_geometry's.  n_hits may exceed hit_off[n] (the slots behind are ignored).  q == 0 or n_hits == 0 (n == 0 among
 * them): the q + 1 offsets are zeroed and nothing else is written.  FMX_E_ARG for null or negative arguments, a bad query_off, a
 * negative term_len, a workspace that is too small (nothing is launched, nothing is written), an index without a line table
 * (fmx_last_error names fmx_line_table_build), n_hits > 2^31 - 1, a SuffixArray / RrrVector / stand-alone wavelet handle;
 * FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_sequence_lines_scratch_bytes(int32_t n, int32_t q, int64_t n_hits);
int fmx_sequence_lines_of_hits_dev(const fmx_index *idx, int32_t n, int32_t q, const int32_t *query_off, const int32_t *term_len,
                                   const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int32_t max_lines,
                                   int64_t *d_line_off, int32_t *d_lines, int32_t *d_line_count, int32_t *d_spans, void *d_ws,
                                   size_t ws_bytes, void *stream);
/* THE VALUES THAT FOLLOW A PATTERN over device pointers, after the two packed stages of the literal or the class search:
 * (d_hit_off, d_locs) hold the hits of n patterns, exactly what the locate stage reports (quirk rows included); term_len[i] >= 0
 * is the length of pattern i.  With textLength = getInputLength() - 1, a hit h of pattern i has
 *     s = min(max(h + term_len[i], 0), textLength),   e = min(s + max_len, textLength),
 *     window = what extract(s, e, destination, 0) stores (fmx_extract_packed_*'s answer, its quirks included),
 *     value  = the window up to, not including, its first code unit that is in the stop set; the whole window if there is none.
 * The empty string is a value (the pattern followed at once by a stop unit, or by the end of the text).  The answer of pattern i
 * is its distinct values, ascending by UTF-16 code unit, a value in front of its extensions ("1" < "10" < "2"), each with the
 * number of hits that have it.  term_len and stop are HOST arrays: validated, and copied into d_ws before the call returns.
 * stage 1, fmx_values_of_hits_dev: d_val_off (n + 1 int64) = where the groups of each pattern begin, d_val_off[n] = G; d_count
 * (room for n_hits ints) = the hits of group g; d_text_off (room for n_hits + 1 int64) = where its code units begin, d_text_off[G]
 * = all of them; d_status (nullable, n ints, read-modify-write: the locate stage's): a window the packed extract ran literally
 * (its redo list) hands the status of that run to its pattern (windows of one pattern with different such statuses: one of them).  Entries behind d_val_off[n], d_count[G - 1] and d_text_off[G] keep
 * the caller's values.  The caller reads G and d_text_off[G] between the stages and gives d_chars that many code units.
 * stage 2, fmx_values_fill_dev: the code units of the G groups into d_chars, from the same d_ws, untouched in between.
 * The stages hand lanes to hits, runs or groups: the windows (a lane per hit), the packed extract over them (lanes per piece),
 * the values' lengths (the stop set in LDS), RUNS of neighbouring hits with one value — the hits of a pattern stand in SA-row
 * order, that is ordered by the text behind the pattern —, then the exact grouping of the runs by stable radix-sort passes over
 * (length; chunks of four code units, last to first, padded with 0; pattern), heads, scans.  Integers only, no atomics, no
 * hashes: the result does not depend on scheduling.  On an index built without extraction: no values, every d_status entry
 * FMX_ST_NOT_ENABLED.
 * d_ws: at least fmx_values_of_hits_scratch_bytes(n, n_hits, max_len) bytes (about 170 + 2 * max_len per hit: the windows' ranges,
 * offsets and text, the packed extract's own workspace, lengths, runs, two permutations and two key arrays, the heads' scans —
 * plus rocPRIM's temporary storage; 0 for an empty call or a shape the call refuses).  The grids are fmx_hit_lines_geometry's; the
 * extract's honour the options "block" and "groups_per_cu".  n_hits may exceed d_hit_off[n] (the slots behind are ignored).
 * n == 0 or n_hits == 0: the n + 1 offsets and d_text_off[0] are zeroed and nothing else is written.  FMX_E_ARG for null or negative
 * arguments, max_len outside [1, 64], n_stop outside [0, 64], a negative term_len, n_hits > 2^31 - 1, n_hits * max_len > 2^35, a
 * workspace that is too small (nothing is launched, nothing is written), a SuffixArray / RrrVector / stand-alone wavelet handle;
 * FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_values_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len);
int fmx_values_of_hits_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                           const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_val_off, int32_t *d_count,
                           int64_t *d_text_off, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);
int fmx_values_fill_dev(const fmx_index *idx, int64_t n_groups, const int64_t *d_text_off, uint16_t *d_chars, const void *d_ws,
                        size_t ws_bytes, void *stream);
/* THE HITS THAT LIE IN GIVEN LINES over device pointers: packed hits (d_hit_off, d_locs) of n patterns -> the same packed format
 * (d_kept_off, d_kept_locs) with the hits that pass, so that the line, sequence and values stages run unchanged on the filtered
 * hits.  (d_line_off, d_lines) are the packed lines of q queries, ascending and distinct per query: what fmx_lines_of_hits_dev,
 * fmx_query_lines_of_hits_dev and fmx_sequence_lines_of_hits_dev leave without a limit.  where_of (n ints, -1 .. q - 1) is a HOST
 * array: validated, and copied into d_ws before the call returns.
 * THE KEEP RULE: a hit h of pattern i is kept iff L = the line of h (a hit belongs to the line of its first character:
 * fmx_lines_of_hits_dev's rule) satisfies line_lo <= L < line_hi, and where_of[i] < 0 or L occurs in
 * d_lines[d_line_off[w] .. d_line_off[w + 1]), w = where_of[i].  A window of 0, INT32_MAX does not filter.
 * d_kept_off (n + 1 int64): d_kept_off[0] = 0, d_kept_off[i + 1] - d_kept_off[i] = the kept hits of pattern i.  d_kept_locs (room
 * for n_hits ints, not overlapping d_locs): the kept hits IN THE ORDER THEY HAD — the compaction is stable, the hits of a pattern
 * stay in SA-row order; entries from d_kept_off[n] on keep the caller's values.  d_hit_off[0] may be non-zero: the hits of the
 * call are the slots [d_hit_off[0], min(d_hit_off[n], n_hits)) of d_locs, those in front and behind are ignored — one packed block
 * may hold filter terms and value patterns side by side (hand over d_hit_off + the number of terms).
 * The stages hand lanes to hits: a flag per slot (the hit's pattern from the hit tiles, its line over the fences staged in LDS,
 * ONE binary search in the query's line list), rocPRIM's exclusive scan of the flags, a scatter; a lane per pattern reads
 * d_kept_off off the scan.  Integers only, no atomics: the result does not depend on scheduling.  Asynchronous on `stream`,
 * nothing is synchronised or allocated.  d_ws: at least fmx_hits_in_lines_scratch_bytes(n, n_hits) bytes (8 per slot, 4 per
 * pattern, rocPRIM's temporary storage; 0 for an empty call or n_hits beyond 2^31 - 1).  The grids are fmx_hit_lines_geometry's.
 * n == 0 or n_hits == 0: the n + 1 offsets are zeroed and nothing else is written.  FMX_E_ARG for null or negative arguments,
 * line_lo > line_hi, a where_of outside -1 .. q - 1, n_hits > 2^31 - 1, an index without a line table (the error names
 * fmx_line_table_build), a workspace that is too small (nothing is launched, nothing is written), a SuffixArray / RrrVector /
 * stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_hits_in_lines_scratch_bytes(int32_t n, int64_t n_hits);
int fmx_hits_in_lines_dev(const fmx_index *idx, int32_t n, const int32_t *where_of, int32_t q, const int64_t *d_line_off, const int32_t *d_lines,
                          int32_t line_lo, int32_t line_hi, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                          int64_t *d_kept_off, int32_t *d_kept_locs, void *d_ws, size_t ws_bytes, void *stream);
/* LINES AND HITS PER BUCKET OF LINES over device pointers (the edges and buckets: fmx_line_histogram_batch above).  edges is a HOST
 * array in both forms, as where_of and query_off are: validated, and copied into d_ws before the call returns.  d_hist gets
 * rows * B int32; entries behind them keep the caller's values.
 * fmx_lines_histogram_dev: packed ascending lists (d_line_off, d_lines) of q lists — what the line, query and sequence stages
 * leave without a limit; an entry that occurs twice in a list counts twice — -> d_hist[Q * B + b] = the entries of list Q in bucket
 * b.  A lane per (list, edge) does ONE lower bound of the edge in its list, a lane per (list, bucket) then takes the difference
 * of two neighbouring ranks: q * n_edges short searches — a list of 10^7 lines costs what a list of 10 costs, no lane walks a
 * list.  Needs no line table.  d_ws: at least fmx_lines_histogram_scratch_bytes(q, n_edges) bytes (8 per (list, edge), 4 per edge).
 * fmx_hits_histogram_dev: packed hits (d_hit_off, d_locs, n_hits) of n patterns exactly as fmx_hits_in_lines_dev takes them —
 * d_hit_off[0] may be non-zero, slots behind d_hit_off[n] are ignored; the hits are in SA-row order, not in text order — ->
 * d_hist[i * B + b] = the hits of pattern i whose line (the line of the hit's first character) lies in bucket b.  A lane per slot
 * makes the key pattern | bucket (the pattern from the hit tiles, the line over the fences staged in LDS, the bucket by an upper
 * bound over the edges: up to 4,096 edges are staged in LDS, more are searched in HBM — correct, not tuned; the bucket B stands
 * for "no bucket", the pattern n for a slot that is no hit); ONE device-wide rocPRIM radix sort over the bits in use; a lane per
 * (pattern, bucket) takes two lower bounds in the sorted keys.  d_ws: at least fmx_hits_histogram_scratch_bytes(n, n_hits,
 * n_edges) bytes (16 per slot, 4 per edge, rocPRIM's temporary storage).
 * Both: integers only, no atomics — the result does not depend on scheduling; lanes go to slots or to counters, never to patterns;
 * the grids are fmx_hit_lines_geometry's; asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged
 * host copy of edges.  The scratch sizes are 0 for an empty call or a shape the call refuses.  q == 0, n == 0: nothing is written;
 * n_hits == 0: the n * B counters are zeroed and nothing else is written.
 * FMX_E_ARG for null or negative arguments, n_edges < 2, a negative first edge, decreasing edges, (int64) rows * B above 2^27,
 * n_hits > 2^31 - 1, an index without a line table (hits form only; the error names fmx_line_table_build), a workspace that is too
 * small (nothing is launched, nothing is written), a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a
 * handle that is not resident. */
size_t fmx_lines_histogram_scratch_bytes(int32_t q, int32_t n_edges);
size_t fmx_hits_histogram_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges);
int fmx_lines_histogram_dev(const fmx_index *idx, int32_t q, const int64_t *d_line_off, const int32_t *d_lines, const int32_t *edges,
                            int32_t n_edges, int32_t *d_hist, void *d_ws, size_t ws_bytes, void *stream);
int fmx_hits_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *edges,
                           int32_t n_edges, int32_t *d_hist, void *d_ws, size_t ws_bytes, void *stream);
/* THE NUMBER BEHIND A PATTERN over device pointers (the value of a hit, the rows and the invariant: fmx_number_stats_where_batch
 * above).  Packed hits (d_hit_off, d_locs, n_hits) of n patterns exactly as fmx_hits_histogram_dev takes them — d_hit_off[0] may be
 * non-zero, slots behind d_hit_off[n] and beyond n_hits are no hits, the order is SA-row order.  term_len (n, the patterns'
 * lengths), edges (NULL with n_edges == 0: one bucket, every line, no line table needed) and permille are HOST arrays: validated,
 * and copied into d_ws before the call returns.  d_count, d_sum_lo, d_sum_hi, d_min, d_max get n * B entries, d_pct n * B * P,
 * d_not_number and d_overflow n; each is nullable except d_count; entries behind them keep the caller's values.  d_status
 * (nullable, n ints the caller has initialised): a window the packed extract ran literally hands its status to its pattern; on an
 * index without extraction every status is FMX_ST_NOT_ENABLED and every row and counter zero.
 * A lane per slot makes the window and the key pattern | bucket (fences and up to 4,096 edges staged in LDS, as the hits
 * histogram's key kernel); the packed extract fills all windows (redo launch included); a lane per slot parses its window into an
 * int64 and the key pattern | code, the code in [0, B + 2]: a bucket, B = no bucket, B + 1 = not a number, B + 2 = overflow (the
 * pattern n for a slot that is no hit); two stable rocPRIM radix sorts, by value over 63 bits and by key over the bits in use, give
 * the order (key, value); two inclusive scans of the values' low and high halves give the running sums; a lane per (pattern,
 * bucket) takes two lower bounds in the sorted keys and stores count, min (the first value), max (the last), the 128-bit sum from
 * two differences, the percentiles by index; a lane per pattern stores not_number and overflow the same way.  Integers only, no
 * atomics — the result does not depend on scheduling; lanes go to slots or to counters, never to patterns; the grids are
 * fmx_hit_lines_geometry's and the extract honours `block` and `groups_per_cu`; asynchronous on `stream`, nothing is allocated,
 * nothing is synchronised beyond the staged host copy of the small arrays.  d_ws: at least fmx_numbers_of_hits_scratch_bytes(n,
 * n_hits, n_edges, n_permille) bytes (about 150 per slot: the window's 64, four 8-byte sort arrays, the ranges and offsets, the
 * extract's scratch, rocPRIM's temporary storage); 0 for an empty call or a shape the call refuses.  n == 0: nothing is written;
 * n_hits == 0: the rows and the per-pattern counters are zeroed and nothing else is written.
 * FMX_E_ARG for null or negative arguments, n_hits > 2^31 - 1, (int64) n * B above 2^27, n * B * max(P, 1) above 2^27, frac_digits
 * outside [0, 9], n_permille outside [0, 16], a permille outside [0, 1000], a negative term_len, the edge rules of
 * fmx_hits_histogram_dev, an index without a line table when edges != NULL, a workspace that is too small (nothing is launched,
 * nothing is written), a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_numbers_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_edges, int32_t n_permille);
int fmx_numbers_of_hits_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int64_t *d_hit_off, const int32_t *d_locs,
                            int64_t n_hits, const int32_t *edges, int32_t n_edges, int32_t frac_digits, const int32_t *permille,
                            int32_t n_permille, int32_t *d_count, uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min, int64_t *d_max,
                            int64_t *d_pct, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes,
                            void *stream);
/* THE LINES RANKED BY THE NUMBER BEHIND A PATTERN over device pointers (the value of a hit, the candidate of a line, the ranking
 * and the rows: fmx_top_lines_where_batch above).  Packed hits (d_hit_off, d_locs, n_hits) of n patterns exactly as
 * fmx_numbers_of_hits_dev takes them — d_hit_off has n + 1 entries, d_hit_off[0] may be non-zero, slots in front of it, behind
 * d_hit_off[n] and beyond n_hits are no hits, the order is SA-row order; every hit given is a kept hit (the window of lines is the
 * filter stage's).  term_len (n, the patterns' lengths) and descending (n bytes) are HOST arrays: validated, and copied into d_ws
 * before the call returns.  d_rows, d_lines, d_numbers, d_not_number and d_overflow get n entries, d_row_line, d_row_value and
 * d_row_loc n * top; each is nullable except d_rows; entries behind them keep the caller's values.  d_status (nullable, n ints the
 * caller has initialised): a window the packed extract ran literally hands its status to its pattern; on an index without
 * extraction every status is FMX_ST_NOT_ENABLED and every row and counter zero.
 * A lane per slot makes the window and the key pattern | position (the slice of d_hit_off staged in LDS); the packed extract fills
 * all windows (redo launch included); a lane per slot parses its window into the ordered value u = descending ? INT64_MAX - value :
 * value — a slot that does not parse gets the pattern n, its reason goes into one word of two halves whose exclusive scan gives
 * not_number and overflow of every pattern; ONE rocPRIM radix sort by pattern | position over the bits in use (lines never decrease
 * within a pattern); a lane per sorted slot finds its line (the fences staged in LDS); rocPRIM's reduce_by_key over the runs of
 * equal (pattern, line) keeps the minimum of (u, position) — a lane's work does not grow with the hits of one line; the candidates
 * lie in (pattern, line) order, so one stable sort by u (63 bits) and one stable sort over the pattern's bits rank them, stability
 * being the tie rule; a lane per pattern reads its segment, lines, rows, numbers and the two reasons; a lane per row (i, j) reads
 * rank first + j.  Integers only, no atomics of its own — the result does not depend on scheduling; lanes go to slots, keys or
 * rows, never to patterns or lines; the grids are fmx_hit_lines_geometry's and the extract honours `block` and `groups_per_cu`;
 * asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged host copy of the small arrays.
 * d_ws: at least fmx_top_lines_of_hits_scratch_bytes(n, n_hits, top) bytes (about 250 per slot: the window's 64, four 8-byte sort
 * arrays, the reasons and their scan, the runs' and candidates' keys and pairs, the ranking's index and pattern arrays, the ranges
 * and offsets, the extract's scratch, rocPRIM's temporary storage); 0 for an empty call or a shape the call refuses.  n == 0:
 * nothing is written; n_hits == 0: the per-pattern counters and the rows are zeroed and nothing else is written.
 * FMX_E_ARG for null or negative arguments, n_hits > 2^31 - 1, frac_digits outside [0, 9], first < 0, top < 1, (int64) n * top
 * above 2^27, a negative term_len, an index without a line table, a workspace that is too small (nothing is launched, nothing is
 * written), a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_top_lines_of_hits_scratch_bytes(int32_t n, int64_t n_hits, int32_t top);
int fmx_top_lines_of_hits_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const uint8_t *descending, const int64_t *d_hit_off,
                              const int32_t *d_locs, int64_t n_hits, int32_t frac_digits, int32_t first, int32_t top, int32_t *d_rows,
                              int32_t *d_row_line, int64_t *d_row_value, int32_t *d_row_loc, int32_t *d_lines, int32_t *d_numbers,
                              int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);
/* STATISTICS BY KEY over device pointers (the key of a line, the groups, the rows and the invariant: fmx_number_stats_by_batch
 * above), three stages on one stream; the caller reads stage b's m + 1 group offsets between b and c, as it reads G between
 * fmx_values_of_hits_dev and fmx_values_fill_dev.  Integers only, no atomics — the results do not depend on scheduling; lanes go to
 * hits, keys or rows, never to patterns; the grids are fmx_hit_lines_geometry's and the extract honours `block` and
 * `groups_per_cu`; asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged host copy of the small
 * arrays.  Every stage refuses with FMX_E_ARG, before anything is launched or written: null or negative arguments, n_hits > 2^31 -
 * 1, a workspace smaller than its _scratch_bytes function says (which is 0 for an empty call or a shape the call refuses), a
 * SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident.
 *
 * STAGE a, fmx_first_hits_of_lines_dev: THE FIRST HIT OF EVERY LINE.  Packed hits (d_hit_off, d_locs, n_hits) of m patterns as
 * fmx_hits_in_lines_dev takes them — d_hit_off[0] may be non-zero, slots in front of it, behind d_hit_off[m] and beyond n_hits are
 * no hits, any order; positions in [0, textLength] — go to d_first_off (m + 1 int64, d_first_off[0] = 0), d_first_lines and
 * d_first_locs (room for the hits of the m patterns; entries behind d_first_off[m] keep the caller's values): per pattern its
 * distinct lines ascending, each with the smallest position of a hit on it.  A lane per slot makes the key pattern | position; ONE
 * rocPRIM radix sort over the bits in use; a lane per sorted slot finds its line (fences staged in LDS); a lane per sorted slot
 * compares pattern and line with its predecessor's; an exclusive scan; a head stores its line and position.  About 30 bytes of
 * workspace per slot.  m == 0: nothing is written; n_hits == 0: d_first_off is zeroed.  FMX_E_ARG also for an index without a
 * line table.
 *
 * STAGE b, fmx_values_of_hits_groups_dev: fmx_values_of_hits_dev — its arguments, outputs, limits and refusals, d_hit_off[0] = 0 —
 * with one more output, d_group_of_hit (n_hits ints): the index of each hit's group within its pattern (d_val_off[p] + it = the
 * group), -1 for a slot that is no hit.  The grouping is exact for hits in any order, so it runs over stage a's hits, which stand
 * in line order: d_count[g] is then the number of LINES that have key g.  Its workspace is its own
 * (fmx_values_of_hits_groups_scratch_bytes: fmx_values_of_hits_scratch_bytes and four bytes per hit); fmx_values_fill_dev takes it
 * unchanged.  On an index without extraction there are no groups, every d_group_of_hit is -1 and every status FMX_ST_NOT_ENABLED.
 * fmx_values_of_hits_dev and fmx_values_of_hits_scratch_bytes answer what they always did.
 *
 * STAGE c, fmx_numbers_by_key_dev: THE ROWS.  Packed hits of n number patterns as fmx_numbers_of_hits_dev takes them.  term_len (n),
 * by_of (n, each in [0, m)), val_off (m + 1: stage b's d_val_off, read by the caller) and permille are HOST arrays: validated, and
 * copied into d_ws before the call returns.  d_first_off, d_first_lines: stage a's; d_group_of_first: stage b's d_group_of_hit over
 * them.  d_row_off (n + 1 int64) gets the rows' offsets, R = d_row_off[n] = the sum over i of the groups of by_of[i]; d_count,
 * d_sum_lo, d_sum_hi, d_min, d_max get R entries, d_pct R * P, d_no_key, d_not_number and d_overflow n; each nullable except
 * d_row_off and (with R > 0) d_count; entries behind them keep the caller's values.  d_status as in fmx_numbers_of_hits_dev.  A
 * lane per slot makes the window, finds its line and takes ONE lower bound in the first lines of its key pattern: the code of the
 * slot is the group of the found first hit, B = the largest group count of the call for NO KEY, B + 1 not a number, B + 2 overflow;
 * then the packed extract, the parse, the two stable sorts and the two running sums of fmx_numbers_of_hits_dev; a lane per PACKED
 * row finds its pattern in the row offsets and takes the two lower bounds; a lane per pattern stores the three counters.
 * n == 0: nothing is written; n_hits == 0 or an index without extraction: d_row_off is stored, the rows and the counters are
 * zeroed (without extraction every status is FMX_ST_NOT_ENABLED).  FMX_E_ARG also for frac_digits outside [0, 9], n_permille
 * outside [0, 16], a permille outside [0, 1000], a negative term_len, m == 0 with n > 0, a by_of outside [0, m), a val_off that
 * starts below 0 or decreases, R above 2^27, R * max(P, 1) above 2^27, an index without a line table. */
size_t fmx_first_hits_of_lines_scratch_bytes(int32_t m, int64_t n_hits);
int fmx_first_hits_of_lines_dev(const fmx_index *idx, int32_t m, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits,
                                int64_t *d_first_off, int32_t *d_first_lines, int32_t *d_first_locs, void *d_ws, size_t ws_bytes, void *stream);
size_t fmx_values_of_hits_groups_scratch_bytes(int32_t n, int64_t n_hits, int32_t max_len);
int fmx_values_of_hits_groups_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const uint16_t *stop, int32_t n_stop, int32_t max_len,
                                  const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_val_off, int32_t *d_count,
                                  int64_t *d_text_off, int32_t *d_group_of_hit, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);
size_t fmx_numbers_by_key_scratch_bytes(int32_t n, int64_t n_hits, int32_t n_permille);
int fmx_numbers_by_key_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int32_t *by_of, int32_t m, const int64_t *val_off,
                           const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int64_t *d_first_off,
                           const int32_t *d_first_lines, const int32_t *d_group_of_first, int32_t frac_digits, const int32_t *permille,
                           int32_t n_permille, int64_t *d_row_off, int32_t *d_count, uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min,
                           int64_t *d_max, int64_t *d_pct, int32_t *d_no_key, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status,
                           void *d_ws, size_t ws_bytes, void *stream);
/* STATISTICS BY TWO KEYS over device pointers (the pair key, the pairs and the invariants: fmx_number_stats_by_pair_batch above):
 * ONE join stage on one stream between stages b and c of STATISTICS BY KEY.  fmx_pairs_of_first_hits_dev takes stage a's
 * d_first_off (m + 1) and d_first_lines and stage b's d_group_of_hit over them as d_group_of_first; val_off (m + 1: stage b's
 * d_val_off, read by the caller), pair_a and pair_b (n_pairs = c, each in [0, m)) are HOST arrays: validated, and copied into d_ws
 * before the call returns.  n_slots: the caller's upper bound of the first hits of the a-sides, pair_a[0] .. pair_a[c - 1], added
 * up (the kept hits of those key patterns will do).  Outputs: d_pair_off (c + 1 int64); d_pair_group_a, d_pair_group_b, d_pair_lines
 * (entry r of pair j at d_pair_off[j] + r; room for n_slots each, entries behind d_pair_off[c] keep the caller's values); and THE
 * JOINED LISTS in the form of the inputs: d_joined_off (c + 1 int64), d_joined_lines (per pair the lines with a pair key,
 * ascending) and d_joined_group (the index of that line's pair among the pairs of j), room for n_slots each, entries behind
 * d_joined_off[c] keep the caller's values.  fmx_numbers_by_key_dev takes the joined lists as (d_first_off, d_first_lines,
 * d_group_of_first) with m := c and val_off := d_pair_off, read by the caller; by_of then names pairs.
 * A lane per a-side slot finds its pair in the slots' offsets (runs of equal offsets: a pair whose a-side is empty) and takes ONE
 * lower bound of its line in the b-side's first lines; its key is pair | ga | gb, a slot without a partner and every slot behind
 * the real ones gets a key that sorts last; ONE stable rocPRIM radix sort of (key, slot) over the bits in use; a lane per sorted
 * slot flags the head of a run of equal keys; a scan; a head stores ga, gb and the run's length (a binary search: no lane's work
 * grows with the lines of a pair); a lane per sorted slot writes its pair's index back to its slot; a scan and a stable
 * compaction over the slots in their original order leave the joined lists.  Integers only, no atomics; the grids are
 * fmx_hit_lines_geometry's over n_slots; asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged
 * host copy of the small arrays.  About 40 bytes of workspace per slot.  n_pairs == 0: nothing is written; n_slots == 0: d_pair_off
 * and d_joined_off are zeroed.  No line table is needed.
 * FMX_E_ARG, before anything is launched or written and before the handle is asked for its device: null or negative arguments, a
 * pair_a / pair_b outside [0, m), n_pairs > 0 with m == 0, a val_off that starts below 0, decreases or holds more than 2^31 - 1
 * groups of one key pattern, n_slots > 2^31 - 1, fm_bits(c) + fm_bits(the most groups of an a-side) + fm_bits(the most groups of a
 * b-side) > 64, a workspace smaller than fmx_pairs_of_first_hits_scratch_bytes says (which is 0 for an empty call or a shape the
 * call refuses); then a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_pairs_of_first_hits_scratch_bytes(int32_t m, int32_t n_pairs, int64_t n_slots);
int fmx_pairs_of_first_hits_dev(const fmx_index *idx, int32_t m, const int64_t *val_off, int32_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                                const int64_t *d_first_off, const int32_t *d_first_lines, const int32_t *d_group_of_first, int64_t n_slots,
                                int64_t *d_pair_off, int32_t *d_pair_group_a, int32_t *d_pair_group_b, int32_t *d_pair_lines, int64_t *d_joined_off,
                                int32_t *d_joined_lines, int32_t *d_joined_group, void *d_ws, size_t ws_bytes, void *stream);
/* STATISTICS BY KEY PER BUCKET over device pointers (the key rows, the cells and the invariants:
 * fmx_number_stats_by_histogram_batch above): ONE stage on one stream behind stages a and b of STATISTICS BY KEY; the caller reads
 * stage b's m + 1 group offsets in front of it.  Integers only, no atomics, no hashes — the results do not depend on scheduling;
 * lanes go to groups, slots, cells or code units, never to patterns; the grids are fmx_hit_lines_geometry's and the extract honours
 * `block` and `groups_per_cu`; asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged host copy
 * of the small arrays (term_len, by_of, val_off, edges, permille: HOST arrays, validated, copied into d_ws before the call returns).
 * Packed hits (d_hit_off, d_locs, n_hits) of n number patterns as fmx_numbers_by_key_dev takes them; d_first_off, d_first_lines:
 * stage a's; d_group_of_first and d_group_lines (G = val_off[m] ints): stage b's d_group_of_hit and d_count over them.
 * d_key_row_off (m + 1 int64), d_key_row_group and d_key_row_lines (R = the sum of min(top, G_k)), d_cell_off (n + 1 int64),
 * d_count, d_sum_lo, d_sum_hi, d_min, d_max (d_cell_off[n] entries, = the sum over i of (R_by_of[i] + 1) * B), d_pct (that times P),
 * d_no_key, d_not_number and d_overflow (n) get the answer; the cells' arrays are nullable except d_count; entries behind them keep
 * the caller's values.  d_status as in fmx_numbers_of_hits_dev.
 *   1. rank: a lane per group makes the key (key pattern << 31) | (INT32_MAX - lines), 31 + fm_bits(m) bits; ONE stable rocPRIM
 *      radix sort carries the group's index; a lane per sorted group stores rank_of_group = min(sorted index - val_off[k], top) and,
 *      below top, the key row's group and lines.  Stability is the tie rule.
 *   2. codes: a lane per slot makes its window, finds its pattern (tiles of 1,024 slots, a slice of d_hit_off in LDS), its line
 *      (4,096 fences in LDS), its bucket (up to 4,096 edges in LDS, more are searched in HBM; none: bucket 0) and takes ONE lower
 *      bound in the first lines of its key pattern; the code is min(rank_of_group, R_k) * B + bucket, and with C = (min(top, max_k
 *      G_k) + 1) * B the codes C = no key, C + 1 = not a number, C + 2 = overflow; 48 KiB of LDS per workgroup of 1,024 lanes.  A
 *      hit whose line lies in no bucket has no cell and is counted with no_key: hand in hits of the edges' span only (the host form's
 *      filter does).
 *   3. the packed extract, the parse, the two stable sorts (value over 63 bits, then pattern | code) and the two running sums of
 *      fmx_numbers_of_hits_dev, as they are.
 *   4. cells: a lane per PACKED cell finds its pattern in the cell offsets and takes the two lower bounds, then reads count, min,
 *      max, the 128-bit sum and the percentiles; a lane per number pattern stores the three counters.
 * The text of the key rows is fmx_values_fill_dev and fmx_values_gather_rows_dev as they are, over (m, val_off, top, d_key_row_group).
 * Workspace: fmx_numbers_by_key_scratch_bytes' per slot, 28 bytes per group, and rocPRIM's.  n == 0: nothing is written;
 * n_hits == 0 or an index without extraction: the key rows and both offset arrays are stored, the cells and the counters are zeroed
 * (without extraction every status is FMX_ST_NOT_ENABLED; the workspace is then sized for n_hits = 0).  FMX_E_ARG, before
 * anything is launched or written: null or negative arguments, n_hits > 2^31 - 1, frac_digits outside [0, 9], n_permille outside
 * [0, 16], a permille outside [0, 1000], a negative term_len, bad edges, top outside [1, 65536], (int64) n * (top + 1) * B above
 * 2^27 or that times max(P, 1) above 2^27, m == 0 with n > 0, a by_of outside [0, m), a val_off that does not start at 0, decreases
 * or holds more than 2^31 - 1 groups, a workspace smaller than fmx_numbers_by_key_buckets_scratch_bytes says (which is 0 for a
 * shape the call refuses), an index without a line table, a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE
 * for a handle that is not resident. */
size_t fmx_numbers_by_key_buckets_scratch_bytes(int32_t n, int32_t m, int64_t n_groups, int64_t n_hits, int32_t n_edges, int32_t n_permille);
int fmx_numbers_by_key_buckets_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int32_t *by_of, int32_t m, const int64_t *val_off,
                                   int32_t top, const int32_t *edges, int32_t n_edges, const int64_t *d_hit_off, const int32_t *d_locs,
                                   int64_t n_hits, const int64_t *d_first_off, const int32_t *d_first_lines, const int32_t *d_group_of_first,
                                   const int32_t *d_group_lines, int32_t frac_digits, const int32_t *permille, int32_t n_permille,
                                   int64_t *d_key_row_off, int32_t *d_key_row_group, int32_t *d_key_row_lines, int64_t *d_cell_off, int32_t *d_count,
                                   uint64_t *d_sum_lo, uint64_t *d_sum_hi, int64_t *d_min, int64_t *d_max, int64_t *d_pct, int32_t *d_no_key,
                                   int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws, size_t ws_bytes, void *stream);
/* TOP VALUES PER BUCKET over device pointers (the rows, `other` and the invariants: fmx_field_values_histogram_where_batch above),
 * two stages on one stream behind fmx_values_of_hits_groups_dev; the caller reads that stage's n + 1 group offsets in front of
 * them.  Integers only, no atomics, no hashes — the results do not depend on scheduling; lanes go to groups, slots, counters or code
 * units, never to patterns; the grids are fmx_hit_lines_geometry's; asynchronous on `stream`, nothing is allocated, nothing is
 * synchronised beyond the staged host copy of the small arrays.  Both refuse with FMX_E_ARG, before anything is launched or
 * written: null or negative arguments, n_hits > 2^31 - 1, top outside [1, 65536], a val_off that does not start at 0, decreases or
 * holds more than 2^31 - 1 groups, a workspace smaller than the _scratch_bytes function says (which is 0 for an empty call or a shape
 * the call refuses), a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident.
 * Nothing is tuned in this version: the block sizes and grids are the hits histogram's.
 *
 * fmx_values_top_histogram_dev: THE RANKS, THE ROWS AND THE COUNTERS.  val_off (n + 1: fmx_values_of_hits_groups_dev's d_val_off,
 * read by the caller) and edges (as fmx_numbers_of_hits_dev takes them: NULL with n_edges == 0 is B = 1, every line, no line table
 * needed) are HOST arrays: validated, and copied into d_ws before the call returns.  Packed hits (d_hit_off, d_locs, n_hits) as
 * fmx_hits_histogram_dev takes them — d_hit_off[0] may be non-zero, slots in front of it, behind d_hit_off[n] and beyond n_hits are
 * no hits; d_count (G = val_off[n] ints) and d_group_of_hit (n_hits ints, indexed by slot) are fmx_values_of_hits_groups_dev's over
 * those hits; a slot whose group is outside its pattern's groups counts as "other".  d_row_off (n + 1 int64), d_row_group and
 * d_row_count (R = the sum of min(top, G_i)), d_hist (R * B) and d_other (n * B) get the answer; entries behind them keep the
 * caller's values.  A hit whose line lies in no bucket is in d_row_count (the group's count) and in no counter.
 *   1. rank: a lane per group makes the key (pattern << 31) | (INT32_MAX - count), 31 + fm_bits(n) bits; ONE stable rocPRIM radix
 *      sort carries the group's index; a lane per sorted group stores rank_of_group = min(sorted index - val_off[pattern], top) and,
 *      below top, the row's group and count;
 *   2. keys: a lane per slot finds its pattern (tiles of 1,024 slots, a slice of d_hit_off in LDS), its line (4,096 fences in LDS),
 *      its bucket (up to 4,096 edges in LDS, more are searched in HBM) and makes the key pattern | rank in [0, top] | bucket in
 *      [0, B]: fm_bits(n) + fm_bits(top) + fm_bits(B) bits, at most 31 + 17 + 28 — a key wider than 64 bits is refused (the limit
 *      on n * (top + 1) * B keeps every accepted call below); 48 KiB of LDS per workgroup of 1,024 lanes;
 *   3. sort: ONE rocPRIM radix sort over the bits in use;
 *   4. counters: a lane per counter, (row, bucket) or (pattern, other, bucket), takes two lower bounds inside its pattern's slots.
 * Workspace: 16 bytes per slot, 28 per group, and rocPRIM's.  n == 0: nothing is written; n_hits == 0: d_row_off and d_other are
 * zeroed.  FMX_E_ARG also for (int64) n * (top + 1) * B above 2^27, bad edges, an index without a line table when edges are given.
 *
 * fmx_values_gather_rows_dev: THE TEXT OF THE ROWS.  After fmx_values_fill_dev has filled the text of ALL groups (d_text_off: G + 1,
 * d_chars), the R selected groups' text goes to d_row_text_off (R + 1 int64) and d_row_chars, packed in row order: a lane per row
 * finds its group (val_off[pattern] + d_row_group[r]) and its length, an exclusive scan, a lane per code unit copies one unit.
 * val_off and top as above (HOST; copied into d_ws); max_units: a bound of the packed length that sizes the grid and d_row_chars'
 * room (the units of all groups, d_text_off[G], will do); nothing is stored behind d_row_text_off[R] units.  No wait: the caller
 * that needs the packed length reads the 8 bytes of d_row_text_off[R] — ONE wait — or sizes its buffer by the bound.  R == 0:
 * d_row_text_off[0] is zeroed. */
size_t fmx_values_top_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges);
int fmx_values_top_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, int32_t top, const int32_t *edges, int32_t n_edges,
                                 const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *d_count,
                                 const int32_t *d_group_of_hit, int64_t *d_row_off, int32_t *d_row_group, int32_t *d_row_count, int32_t *d_hist,
                                 int32_t *d_other, void *d_ws, size_t ws_bytes, void *stream);
size_t fmx_values_gather_rows_scratch_bytes(int32_t n, int64_t n_rows);
int fmx_values_gather_rows_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, int32_t top, int64_t max_units, const int32_t *d_row_group,
                               const int64_t *d_text_off, const uint16_t *d_chars, int64_t *d_row_text_off, uint16_t *d_row_chars, void *d_ws,
                               size_t ws_bytes, void *stream);
/* DISTINCT VALUES PER BUCKET over device pointers (distinct, first_seen and the invariants:
 * fmx_distinct_values_histogram_where_batch above), one stage on one stream behind fmx_values_of_hits_groups_dev; the caller reads
 * that stage's n + 1 group offsets in front of it.  val_off, edges, the packed hits (d_hit_off, d_locs, n_hits) and d_group_of_hit
 * are fmx_values_top_histogram_dev's; d_distinct and d_first_seen get n * B ints each, entries behind them keep the caller's
 * values.  A slot that is no hit, a hit whose line lies in no bucket and a hit whose group is outside its pattern's groups (-1)
 * count nowhere: the first_seen of a group without a hit in a bucket is 0 everywhere.
 *   1. keys: a lane per slot finds its pattern, its line and its bucket as fmx_values_top_histogram_dev's step 2 does and makes the
 *      key pattern | group | bucket, fm_bits(n) + fm_bits(max G_i) + fm_bits(B) bits: n * B <= 2^27 and G <= 2^31 - 1 keep it at 60
 *      bits or below; what counts nowhere gets the pattern n, which sorts last;
 *   2. sort: ONE rocPRIM radix sort over the bits in use;
 *   3. heads: a lane per sorted slot; the head of a run of equal keys becomes (pattern | bucket) << 1 | (0 where it is the first
 *      bucket of its (pattern, group), else 1), every other slot the pattern n;
 *   4. sort: ONE rocPRIM radix sort over fm_bits(n) + fm_bits(B) + 1 bits;
 *   5. counters: a lane per (pattern, bucket) takes three lower bounds over all slots.
 * Integers only, no atomics; lanes go to slots and counters, never to patterns; the grids are fmx_hit_lines_geometry's;
 * asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged host copy of the small arrays.  Nothing
 * is tuned in this version.  Workspace: 32 bytes per slot and rocPRIM's.  n == 0: nothing is written; n_hits == 0: both outputs are
 * zeroed.  FMX_E_ARG, before anything is launched or written: null or negative arguments, n_hits > 2^31 - 1, a val_off that does
 * not start at 0, decreases or holds more than 2^31 - 1 groups, bad edges, (int64) n * B above 2^27, an index without a line table
 * when edges are given, a workspace smaller than fmx_values_distinct_histogram_scratch_bytes says (which is 0 for an empty call or
 * a shape the call refuses), a SuffixArray / RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not
 * resident. */
size_t fmx_values_distinct_histogram_scratch_bytes(int32_t n, int64_t n_groups, int64_t n_hits, int32_t n_edges);
int fmx_values_distinct_histogram_dev(const fmx_index *idx, int32_t n, const int64_t *val_off, const int32_t *edges, int32_t n_edges,
                                      const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, const int32_t *d_group_of_hit,
                                      int32_t *d_distinct, int32_t *d_first_seen, void *d_ws, size_t ws_bytes, void *stream);
/* THE HITS WHOSE NUMBER LIES IN A RANGE over device pointers (ranged patterns, the value of a hit and when it passes:
 * fmx_match_query_number_batch above).  Packed hits (d_hit_off, d_locs, n_hits) of n patterns exactly as fmx_hits_in_lines_dev takes
 * them — d_hit_off[0] may be non-zero, slots behind d_hit_off[n] and beyond n_hits are no hits, the order is SA-row order — and the
 * output is the packed format of the input, as fmx_hits_in_lines_dev leaves it: d_kept_off (n + 1 int64, d_kept_off[0] = 0),
 * d_kept_locs (room for n_hits ints, not overlapping d_locs): the passing hits IN THE ORDER THEY HAD, every hit of an unranged
 * pattern among them; entries from d_kept_off[n] on keep the caller's values.  term_len (n, the patterns' lengths), num_lo and
 * num_hi (n int64 each) are HOST arrays: validated, and copied into d_ws before the call returns.  d_kept, d_not_number, d_overflow
 * (each nullable, n ints): per pattern the hits that pass and those that did not parse, by reason (unranged: every hit, 0, 0).
 * d_status (nullable, n ints the caller has initialised): a window the packed extract ran literally hands its status to its
 * pattern.  On an index built without extraction nothing is launched over the image: every ranged pattern gets
 * FMX_ST_NOT_ENABLED and keeps no hit, unranged patterns are copied through.  No line table is needed.
 * A lane per slot stores the slot's pattern and its window (the hit tiles' loop, 16 KiB of LDS) — an EMPTY window for a slot of an
 * unranged pattern and for a slot that is no hit, so the packed extract walks nothing for them and a call whose ranged terms are
 * rare pays for those hits only; the packed extract fills the windows (redo launch included); a lane per slot parses its window,
 * compares, and stores the flag and the word of the two reasons; two rocPRIM exclusive scans; fmx_hits_in_lines_dev's stable store;
 * a lane per pattern reads the three counters off the scans.  Integers only, no atomics — the result does not depend on
 * scheduling; lanes go to slots, never to patterns; the grids are fmx_hit_lines_geometry's and the extract honours `block` and
 * `groups_per_cu`; asynchronous on `stream`, nothing is allocated, nothing is synchronised beyond the staged host copy of the small
 * arrays.  d_ws: at least fmx_hits_in_number_range_scratch_bytes(n, n_hits) bytes (about 130 per slot: the window's 64, the ranges
 * and offsets, flags and scans, the extract's scratch, rocPRIM's temporary storage; 0 for an empty call or n_hits beyond
 * 2^31 - 1).  n == 0 or n_hits == 0: the n + 1 offsets and the counters are zeroed and nothing else is written.
 * FMX_E_ARG for null or negative arguments, a negative term_len, frac_digits outside [0, 9], n_hits > 2^31 - 1, a workspace that is
 * too small (the error names fmx_hits_in_number_range_scratch_bytes; nothing is launched, nothing is written), a SuffixArray /
 * RrrVector / stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident. */
size_t fmx_hits_in_number_range_scratch_bytes(int32_t n, int64_t n_hits);
int fmx_hits_in_number_range_dev(const fmx_index *idx, int32_t n, const int32_t *term_len, const int64_t *num_lo, const int64_t *num_hi,
                                 int32_t frac_digits, const int64_t *d_hit_off, const int32_t *d_locs, int64_t n_hits, int64_t *d_kept_off,
                                 int32_t *d_kept_locs, int32_t *d_kept, int32_t *d_not_number, int32_t *d_overflow, int32_t *d_status, void *d_ws,
                                 size_t ws_bytes, void *stream);
/* CLASS PATTERNS over device pointers (d_alt, d_pos_off, d_pat_off: the three packed arrays of fmx_count_class_batch, in device
 * memory and trusted as the literal device forms trust theirs); asynchronous on `stream`, nothing is allocated or synchronised.
 * THE SEARCH keeps, per pattern, a frontier of SA ranges: the last position gives {C[c], C[c + 1]} of each of its codes, every
 * further position advances every range by every one of its codes with the two rank calls the literal search makes (FM:469-470).
 * A range with start >= end dies at once (FM:464); an alternative the alphabet lacks matches nothing (FM:458-460, 466-468);
 * duplicate alternatives count once.  THE RANGES of pattern i are what is left after its first position: one {start, end} pair per
 * literal string with hits, bit for bit the pair fmx_locate_all_ranges_dev leaves in d_range_ws for that literal, ascending by
 * start.  Adjacent ranges are not merged and the suffix table is not asked in this version.
 * STATUSES: a pattern without positions gets FMX_ST_JAVA_AIOOBE; a position without alternatives matches nothing (count 0,
 * FMX_ST_OK); a pattern whose frontier is larger than max_ranges after any position, or that has a position of more than
 * FMX_CLASS_ALTS_MAX alternatives, gets FMX_ST_TOO_MANY_RANGES, count 0 and no ranges — whatever the launch shape and the image
 * form.  max_ranges is in [1, FMX_CLASS_RANGES_MAX]: the frontier lives in LDS, two buffers of max_ranges pairs per pattern.
 * stage 1: d_range_off (n + 1 int64) = the exclusive sum of the patterns' range counts, d_range_off[n] = m, the ranges of the
 * batch; d_counts (nullable, n ints) = the sum of end - start over a pattern's ranges = the sum of the literals' count();
 * d_status (nullable, n ints).  scratch: at least fmx_class_ranges_scratch_bytes(n) bytes (256-byte aligned).
 * The caller reads m between the stages and gives d_ranges 2 * m ints.
 * stage 2: the same search again — the price of a layout that does not depend on scheduling — stores the ranges of pattern i at
 * d_ranges[2 * d_range_off[i] ..).  Same arguments as stage 1.
 * fmx_class_hit_offsets_dev: d_range_hit_off (m + 1 int64) = the packed layout of the m ranges' hits, every hit (what
 * fmx_locate_all_ranges_dev leaves for m patterns with max_matches -1), and d_hit_off[i] = d_range_hit_off[d_range_off[i]] for i in
 * 0 .. n.  scratch: fmx_class_hit_offsets_scratch_bytes(m).  After it fmx_locate_all_fill_dev(idx, m, d_range_hit_off, d_ranges, ...)
 * fills the hits, and (d_hit_off, d_locs) is what fmx_lines_of_hits_dev and fmx_query_lines_of_hits_dev take for n patterns or terms.
 * fmx_class_fold_status_dev: d_status[i] |= d_range_status[r] for the ranges r of pattern i (the walk statuses the fill ORs per range).
 * FMX_E_ARG for null or negative arguments, max_ranges outside its interval, m above 2^31 - 1, a scratch that is too small (nothing
 * is launched) and a SuffixArray, RrrVector or stand-alone wavelet handle; FMX_E_NO_DEVICE for a handle that is not resident.
 * n == 0: stage 1 zeroes d_range_off[0], the others do nothing (fmx_class_hit_offsets_dev zeroes d_hit_off[0] and
 * d_range_hit_off[0]). */
size_t fmx_class_ranges_scratch_bytes(int32_t n);
int fmx_class_ranges_count_dev(const fmx_index *idx, const uint16_t *d_alt, const int32_t *d_pos_off, const int32_t *d_pat_off, int32_t n,
                               int32_t max_ranges, int64_t *d_range_off, int32_t *d_counts, int32_t *d_status, void *scratch,
                               size_t scratch_bytes, void *stream);
int fmx_class_ranges_fill_dev(const fmx_index *idx, const uint16_t *d_alt, const int32_t *d_pos_off, const int32_t *d_pat_off, int32_t n,
                              int32_t max_ranges, const int64_t *d_range_off, int32_t *d_ranges, void *stream);
size_t fmx_class_hit_offsets_scratch_bytes(int64_t m);
int fmx_class_hit_offsets_dev(const fmx_index *idx, int32_t n, const int64_t *d_range_off, const int32_t *d_ranges, int64_t m,
                              int64_t *d_range_hit_off, int64_t *d_hit_off, void *scratch, size_t scratch_bytes, void *stream);
int fmx_class_fold_status_dev(const fmx_index *idx, int32_t n, const int64_t *d_range_off, int64_t m, const int32_t *d_range_status,
                              int32_t *d_status, void *stream);
int fmx_extract_batch_dev(const fmx_index *idx, const int32_t *d_start, const int32_t *d_stop, int32_t n,
                          uint16_t *d_dst, int32_t dst_len, int32_t offset, int32_t *d_out_len,
                          int32_t *d_lf_steps, int32_t *d_status, void *stream);
int fmx_extract_boundary_batch_dev(const fmx_index *idx, const int32_t *d_from, int32_t n, uint16_t boundary,
                                   int mode, uint16_t *d_dst, int32_t dst_len, int32_t offset, int32_t *d_out_len,
                                   int32_t *d_lf_steps, int32_t *d_status, int32_t *d_aux, void *stream);

/* ---- locate -> extract pipelines ---------------------------------------------------------------
 * The composite the reference times in locateAndExtractBenchmark (indices/src/jmh/java/com/dynatrace/fm/
 * FmIndexThroughputBenchmark.java:231-249): matches = locate(pattern, 0, length, locations, maxMatches), then
 * for each i < matches extract(locations[i], min(getInputLength(), locations[i] + maxExtractionLength),
 * destination, 0).  Here both stages run on the device and the hit positions never leave HBM.
 * Hit k of pattern i uses slot i*max_matches + k of locs / out_len / hit_status / hit_aux and destination
 * row (i*max_matches + k) of `row length` chars, written from offset 0.  Only slots k < found[i] are
 * written; all others keep the caller's values.  max_matches must be >= 1 (it is the row count per pattern,
 * and the locate limit FM:504-552); n*max_matches must fit an int32.
 *   status[i]     = status of locate(pattern i)              (AIOOBE cannot occur: loc_cap == max_matches)
 *   hit_status[s] = status of the extract call of slot s (e.g. FMX_ST_STOP_TOO_LONG when the hit lies within
 *                   extract_len of the end of the text: the benchmark's stop == getInputLength(), FM:572-574)
 * fmx_locate_lines_* replaces extract by extractUntilBoundary (mode 0) / ...Left (1) / ...Right (2),
 * FM:640-922 — "the lines that contain the pattern"; hit_aux as in fmx_extract_boundary_batch. */
int fmx_locate_extract_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                             int32_t max_matches, int32_t extract_len, int32_t *locs, int32_t *found, uint16_t *dst,
                             int32_t *out_len, int32_t *lf_steps, int32_t *status, int32_t *hit_status);
int fmx_locate_lines_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n,
                           int32_t max_matches, uint16_t boundary, int mode, int32_t dst_len, int32_t *locs,
                           int32_t *found, uint16_t *dst, int32_t *out_len, int32_t *lf_steps, int32_t *status,
                           int32_t *hit_status, int32_t *hit_aux);
/* device-pointer forms: enqueue on `stream`; d_range_ws = 2*n ints; d_hit_status / d_hit_aux may be NULL */
int fmx_locate_extract_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                                 int32_t max_matches, int32_t extract_len, int32_t *d_locs, int32_t *d_found,
                                 uint16_t *d_dst, int32_t *d_out_len, int32_t *d_lf_steps, int32_t *d_status,
                                 int32_t *d_hit_status, int32_t *d_range_ws, void *stream);
int fmx_locate_lines_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                               int32_t max_matches, uint16_t boundary, int mode, int32_t dst_len, int32_t *d_locs,
                               int32_t *d_found, uint16_t *d_dst, int32_t *d_out_len, int32_t *d_lf_steps,
                               int32_t *d_status, int32_t *d_hit_status, int32_t *d_hit_aux, int32_t *d_range_ws,
                               void *stream);

/* ---- segment sets: texts beyond one FmIndex ----------------------------------------------------
 * FmIndex addresses its text with Java ints (`length` FM:131, RrrVector positions RRR:358), so a text of
 * >= 2^31 chars (BASELINE configs[4]: 2 GiB) is K independent FmIndex objects over consecutive pieces of the
 * text, cut at record boundaries; a caller sums count() over them and adds each piece's start to its
 * locate() results.  These entry points do that on the device for K handles resident on the same GPU:
 *   counts[i] = sum over segments of count(pattern i)            (int64: the sum can pass 2^31)
 *   locs      = n rows of max_matches int64 text positions: segment 0's hits (SA order, FM:526-548),
 *               then segment 1's, ... each moved by seg_base[s] (host array), truncated at max_matches;
 *               found[i] = number written (max_matches >= 1)
 *   status[i] = first non-zero per-segment status (an empty pattern fails the same way in every segment)
 * Occurrences that span a cut are not occurrences in any segment, exactly as with K Java objects.
 * Slots of a row at and beyond found[i] keep the caller's values — except in the row of a pattern whose status is non-zero, which is
 * unspecified from found[i] on (a segment's hits are stored straight into the set's rows before its status is known: option
 * "segments_direct").
 * Device forms: d_tmp = 3*n ints (count) / 4*n + n*max_matches ints (locate); d_lf_steps / d_status may be NULL. */
int fmx_count_segments(const fmx_index *const *segs, int32_t n_segs, const uint16_t *pat, const int32_t *pat_off,
                       int32_t n, int64_t *counts, int64_t *lf_steps, int32_t *status);
int fmx_locate_segments(const fmx_index *const *segs, int32_t n_segs, const int64_t *seg_base, const uint16_t *pat,
                        const int32_t *pat_off, int32_t n, int32_t max_matches, int64_t *locs, int32_t *found,
                        int32_t *status);
int fmx_count_segments_dev(const fmx_index *const *segs, int32_t n_segs, const uint16_t *d_pat, const int32_t *d_pat_off,
                           int32_t n, int64_t *d_counts, int64_t *d_lf_steps, int32_t *d_status, int32_t *d_tmp,
                           void *stream);
int fmx_locate_segments_dev(const fmx_index *const *segs, int32_t n_segs, const int64_t *seg_base, const uint16_t *d_pat,
                            const int32_t *d_pat_off, int32_t n, int32_t max_matches, int64_t *d_locs, int32_t *d_found,
                            int32_t *d_status, int32_t *d_tmp, void *stream);
/* count() AND locate() of one batch over a segment set in one pass: the range search of a segment (FM:455-474 = FM:506-523)
 * yields both the count and the SA range its hits are located from, so this costs one search per segment where
 * fmx_count_segments_dev + fmx_locate_segments_dev cost two.  Same outputs as the two calls (d_counts / d_lf_steps: int64 sums
 * over the segments, d_lf_steps may be NULL: the LF-steps of the searches, not of the walks); d_tmp = 4*n + n*max_matches ints. */
int fmx_count_locate_segments_dev(const fmx_index *const *segs, int32_t n_segs, const int64_t *seg_base, const uint16_t *d_pat,
                                  const int32_t *d_pat_off, int32_t n, int32_t max_matches, int64_t *d_counts, int64_t *d_lf_steps,
                                  int64_t *d_locs, int32_t *d_found, int32_t *d_status, int32_t *d_tmp, void *stream);

/* count() AND locate() over a segment set with host buffers (the host form of fmx_count_locate_segments_dev): counts / lf_steps
 * int64 sums over the segments (lf_steps nullable), locs n rows of max_matches int64 (in / out), found, status (nullable). */
int fmx_count_locate_segments(const fmx_index *const *segs, int32_t n_segs, const int64_t *seg_base, const uint16_t *pat,
                              const int32_t *pat_off, int32_t n, int32_t max_matches, int64_t *counts, int64_t *lf_steps,
                              int64_t *locs, int32_t *found, int32_t *status);

/* ---- replicas: one immutable index on several GPUs, one host process ---------------------------------
 * FmIndex is immutable and @ThreadSafe (FM:82; the reference's throughput benchmark gives every thread an index of its own,
 * indices/src/jmh/java/com/dynatrace/fm/FmIndexThroughputState.java:30), and every query of a batch is an independent read: so
 * the image is REPLICATED on the GPUs of a node and a batch is cut into contiguous shards, one per replica — no exchange on the
 * query path, the "gather" is that every shard stores into its own slice of the caller's arrays (SURVEY 8e scheme (i)).
 *
 * fmx_replicate: out[i] = a new handle, resident on devices[i] (i < n_devices; a device may be named more than once — two
 * replicas then share it).  The image goes from where `idx` has it — HBM of its device: one peer copy per destination over
 * xGMI, all destinations at once (root egress over all links, no ring); the host otherwise — and every replica grows its own
 * suffix table and window directory on its device, in parallel.  `idx` itself is unchanged (it may but need not be resident);
 * a replica answers every query and accessor, keeps no host model (fmx_save / fmx_blob: FMX_E_ARG) and is freed with fmx_free.
 * On failure nothing is left behind.  fmx_device_of: the device ordinal a handle is resident on, -1 = not resident. */
int fmx_replicate(const fmx_index *idx, const int32_t *devices, int32_t n_devices, fmx_index **out);
int fmx_device_of(const fmx_index *idx);
/* The shard arithmetic of every *_multi call: items [*lo, *hi) of n belong to part `part` of `parts` (contiguous; sizes differ
 * by at most one, the first n % parts parts hold the extra item). */
void fmx_shard_range(int64_t n, int32_t parts, int32_t part, int64_t *lo, int64_t *hi);

/* The host-buffer batch calls over a replica set: arguments as in the single-index forms; shard r — fmx_shard_range(n,
 * n_replicas, r) — runs on replicas[r] from a host thread of its own (the library keeps one worker per replica slot of a device;
 * the calling thread takes shard 0), all shards at once, each storing into rows / entries [lo, hi) of the caller's arrays.
 * Results are those of the single-index call on the whole batch, entry by entry.  Returns the first failing shard's error
 * (fmx_last_error: its message); the other shards still complete.  Replicas of DIFFERENT indexes are the caller's mistake. */
int fmx_count_batch_multi(const fmx_index *const *replicas, int32_t n_replicas, const uint16_t *pat, const int32_t *pat_off,
                          int32_t n, int32_t *counts, int32_t *lf_steps, int32_t *status);
int fmx_locate_batch_multi(const fmx_index *const *replicas, int32_t n_replicas, const uint16_t *pat, const int32_t *pat_off,
                           int32_t n, int32_t max_matches, int32_t *locs, int32_t loc_cap, int32_t *found, int32_t *lf_steps,
                           int32_t *status);
int fmx_extract_batch_multi(const fmx_index *const *replicas, int32_t n_replicas, const int32_t *start, const int32_t *stop,
                            int32_t n, uint16_t *dst, int32_t dst_len, int32_t offset, int32_t *out_len, int32_t *lf_steps,
                            int32_t *status);
int fmx_extract_boundary_batch_multi(const fmx_index *const *replicas, int32_t n_replicas, const int32_t *from, int32_t n,
                                     uint16_t boundary, int mode, uint16_t *dst, int32_t dst_len, int32_t offset,
                                     int32_t *out_len, int32_t *lf_steps, int32_t *status, int32_t *aux);
/* BASELINE configs[4]: segs = n_replicas x n_segs handles, replica-major (segs[r * n_segs + s] = segment s on replica r's
 * device: fmx_replicate of every segment index onto the same device list); fmx_count_locate_segments per shard. */
int fmx_count_locate_segments_multi(const fmx_index *const *segs, int32_t n_replicas, int32_t n_segs, const int64_t *seg_base,
                                    const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_matches, int64_t *counts,
                                    int64_t *lf_steps, int64_t *locs, int32_t *found, int32_t *status);
/* Device-resident shards, asynchronous: entry r of every array is replica r's operand of fmx_count_batch_dev /
 * fmx_count_locate_segments_dev, resident on that replica's device (n[r] patterns; streams[r] a hipStream_t of that device or
 * NULL).  The launches of all replicas are issued at once, each from its device's worker thread; the call returns when they are
 * ENQUEUED.  fmx_multi_synchronize waits for streams[r] on every replica's device.  (What bench.py --single-process times.) */
int fmx_count_batch_multi_dev(const fmx_index *const *replicas, int32_t n_replicas, const uint16_t *const *d_pat,
                              const int32_t *const *d_pat_off, const int32_t *n, int32_t *const *d_counts,
                              int32_t *const *d_lf_steps, int32_t *const *d_status, void *const *streams);
int fmx_count_locate_segments_multi_dev(const fmx_index *const *segs, int32_t n_replicas, int32_t n_segs, const int64_t *seg_base,
                                        const uint16_t *const *d_pat, const int32_t *const *d_pat_off, const int32_t *n,
                                        int32_t max_matches, int64_t *const *d_counts, int64_t *const *d_lf_steps,
                                        int64_t *const *d_locs, int32_t *const *d_found, int32_t *const *d_status,
                                        int32_t *const *d_tmp, void *const *streams);
int fmx_multi_synchronize(const fmx_index *const *replicas, int32_t n_replicas, void *const *streams);

/* ---- WaveletFixedBlockBoosting as a stand-alone structure (the reference's public class, WFBB:130-154) ----
 * `sequence` = symbols already mapped to small non-negative integers (short[] text of WFBB:130).  The handle
 * answers only the two calls below (after fmx_to_device); free it with fmx_free. */
int fmx_wavelet_build(const int16_t *sequence, int64_t n, int32_t sampling_rate, fmx_index **out);
/* long rank(long position, short symbol) WFBB:1010-1285, batched */
int fmx_wavelet_rank_batch(const fmx_index *idx, const int64_t *positions, const int32_t *symbols, int32_t n,
                           int64_t *ranks, int32_t *status);
/* long inverseSelect(long position) WFBB:1305-1537, batched: packed[i] = (rank << 32) | symbol, and the bare
 * symbol for position 0, exactly as the reference returns it */
int fmx_wavelet_inverse_select_batch(const fmx_index *idx, const int64_t *positions, int32_t n, int64_t *packed,
                                     int32_t *status);

/* ---- RrrVector as a stand-alone structure (the reference's public class, RRR:225-286) -------------------
 * new RrrVector(BitVector, sampleSize): `bits` = one byte per bit.  The handle keeps the vector in its compressed
 * form (15-bit blocks, class + offset) and answers only the two calls below, after fmx_to_device; free it
 * with fmx_free.  (Inside an FM-index image the bit vectors are expanded instead, see fmx_blob.hpp.) */
int fmx_rrr_build(const uint8_t *bits, int64_t n, int32_t sample_size, fmx_index **out);
/* int rankOnes(int position) RRR:358-396, batched (0 below 0, totalOnes from length on) */
int fmx_rrr_rank_ones_batch(const fmx_index *idx, const int32_t *positions, int32_t n, int32_t *ranks);
/* boolean access(int position) RRR:314-349, batched; status = FMX_ST_JAVA_AIOOBE where the reference throws */
int fmx_rrr_access_batch(const fmx_index *idx, const int32_t *positions, int32_t n, uint8_t *bits, int32_t *status);
/* the same two calls with operands resident in HBM, asynchronous on `stream` (RrrVectorThroughputBenchmark.java:43-51 is
 * measured through these: positions in, ranks out, nothing crosses PCIe inside the timed region) */
int fmx_rrr_rank_ones_batch_dev(const fmx_index *idx, const int32_t *d_positions, int32_t n, int32_t *d_ranks, void *stream);
int fmx_rrr_access_batch_dev(const fmx_index *idx, const int32_t *d_positions, int32_t n, uint8_t *d_bits, int32_t *d_status,
                             void *stream);

/* ---- SuffixArray (the reference's public class suffixarray/SuffixArray.java, "SA") --------------------------------
 * The plain suffix-array index: the text and its suffix array of n + 1 entries (entry 0 = n, the empty suffix; then the
 * suffixes in the order of their chars as unsigned 16-bit values, a proper prefix first: SA:56-68, 89-91).
 * fmx_sa_build: build_device >= 0 sorts the suffixes by prefix doubling in that device's HBM and leaves the array there
 * (the handle is then resident on it); build_device = -1 sorts them on the host (SA-IS).  n <= 2^31 - 2.
 * The handle answers the fmx_sa_* calls, fmx_to_device (the resident form: text, array and a fence table made from the
 * options "sa_fences" / "sa_fence_chars"), fmx_free, fmx_input_length and fmx_device_of; every other call refuses it
 * with FMX_E_ARG.  Queries need a resident handle (FMX_E_NO_DEVICE otherwise). */
int fmx_sa_build(const uint16_t *text, int32_t n, int build_device, fmx_index **out);
/* SA:186-199 (raw or ObjectOutputStream-framed): FMX_E_FORMAT unless len(sa) = text length + 1, every entry lies in
 * [0, text length], the stream is complete and its text is well-formed UTF-8; FMX_E_VERSION for another version byte */
int fmx_sa_load(const uint8_t *ser, size_t len, fmx_index **out);
/* SA:172-184; *buf is owned by the library until fmx_free_buffer */
int fmx_sa_save(const fmx_index *idx, int framed, uint8_t **buf, size_t *len);
/* getSuffixArray (SA:164-166): copies min(cap, n + 1) entries; returns n + 1, or a negative FMX_E_* code */
int64_t fmx_sa_get(const fmx_index *idx, int32_t *sa, int64_t cap);
/* hashCode (SA:202-204): String.hashCode(text) + Arrays.hashCode(sa) in int32 arithmetic */
int fmx_sa_hash_code(const fmx_index *idx, int32_t *hash);
/* count (SA:100-104), batched: counts[i] = right - left of the reference's two searches (one fewer than the occurrences
 * when the largest suffix starts with the pattern) */
int fmx_sa_count_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t *counts);
/* locate(p, offsets) (SA:116-129), batched with offsets.length = max_matches: found[i] = min(count, max_matches), and
 * locs[i * max_matches + k] = the array's entry at row left + k for k < found[i] (slots from found[i] on keep their values);
 * counts (nullable) as fmx_sa_count_batch.  n * max_matches < 2^31. */
int fmx_sa_locate_batch(const fmx_index *idx, const uint16_t *pat, const int32_t *pat_off, int32_t n, int32_t max_matches,
                        int32_t *locs, int32_t *found, int32_t *counts);
/* the same with operands in HBM, asynchronous on `stream` */
int fmx_sa_count_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n, int32_t *d_counts,
                           void *stream);
int fmx_sa_locate_batch_dev(const fmx_index *idx, const uint16_t *d_pat, const int32_t *d_pat_off, int32_t n,
                            int32_t max_matches, int32_t *d_locs, int32_t *d_found, int32_t *d_counts, void *stream);

/* BurrowsWheelerTransform.createBurrowsWheelerTransform (BWT:43-113): bwt = n + 1 chars, the transform of text + '\0' (that
 * '\0' an ordinary symbol, tied with any '\0' of the text).  build_device as fmx_sa_build.  FMX_E_ALPHABET when text + '\0'
 * has more than 32,767 distinct chars ("Charset has more than 32767 different characters."). */
int fmx_bwt(const uint16_t *text, int32_t n, int build_device, uint16_t *bwt);

/* ---- helpers ------------------------------------------------------------------------------ */

/* FmIndex.convertBytePatternToCharPattern FM:239-298.  Returns the number of chars, or -1 with
 * *bad_value set when the reference throws "Found a character that exceeds (32767): it was N". */
int fmx_convert_byte_pattern(const uint8_t *pattern, int32_t offset, int32_t length, uint16_t *dest,
                             int32_t *bad_value);
/* the reference's exception message for a status code ("%d" left in place for FMX_ST_DOES_NOT_FIT) */
const char *fmx_status_message(int status);
/* 1 if the exception type is IllegalArgumentException, 0 for RuntimeException, 2 for AIOOBE */
int fmx_status_kind(int status);
const char *fmx_last_error(void);
/* The host-buffer entry points recycle their device scratch between calls (up to 2 GiB per process); this
 * returns it to the driver. */
void fmx_release_scratch(void);
int fmx_device_count(void);
/* Runtime options (process-wide; FMX_E_ARG for an unknown name or a value the option does not take, which then keeps what it had).
 * The complete list — every name with its default, the values it takes and what it does — is the table in
 * index4j_amd/csrc/fmx_options.cpp; tests/test_option_ranges.py pins it.  The groups:
 * launch tunables, read by every launch: workgroup size and grid cap ("block" = 512 | 1024, "groups_per_cu"), which batches are
 * planned and by what (the "sort_*", "plan_*", "walk_*" and "boundary_*" options; fmx_count_batch_is_planned), and A/B switches
 * that force a plainer route ("suffix_table" = 0: launches ignore the index's suffix table, "boundary_accel" = 0: the literal
 * +4-chunk right walk of extractUntilBoundary).  "lf_steps_executed_only" = 1: the LF-step output of count() leaves out the rank
 * evaluations the suffix table answered (bench.py's executed-work figure; the default reports the reference's count).
 * Applied when an index is flattened or becomes resident AFTERWARDS (an index that already is keeps what it has): budget and
 * depth of the suffix table, the LDS cache of superblock headers, the layout of the image (tests force the reference's own routes
 * with it), the window directory of fmx_window_cells_info, the row table of fmx_locate_rows_info, a suffix array's fence table.
 * Applied by fmx_build_on_device: "wavelet_on_device" = 0 encodes the wavelet tree on the host.
 * The "host_*" and "segments_*" options choose how the host-buffer and segment-set entry points stage their copies and streams.
 * Results are identical for every setting. */
/* Image form (fmx_set_option("image_compact", 0 | 1), applies to images flattened afterwards: fmx_to_device / fmx_blob of an index
 * that has none yet).  0 (default): the bit vectors of the wavelet tree and the sampled-row bitmap are EXPANDED into 16-byte cells
 * {ones before, 96 bits} — a rank is one load + three popcounts; 0.64 bytes per text byte resident on the 256 MiB log.
 * 1 (compact): they stay in the reference's own compression (15-bit blocks as class + offset, RRR:225-286) as 16-block records
 * + offsets stream, decoded by the kernels through the value-of-offset table in LDS — smaller (bytes per text byte and timings:
 * DESIGN.md 3), a rank costs a second dependent load.  Results are identical; an image says which form it is, and travels as
 * before (fmx_blob / fmx_attach_device_blob). */
int fmx_set_option(const char *name, int value);

/* deterministic synthetic workload (bench / tests): see index4j_amd/csrc/fmx_synth.cpp */
int fmx_synth_log(uint64_t seed, int32_t n, uint16_t *out);
/* the same log lines with runs of multi-byte characters dropped in at word boundaries (~6 % of the characters), `symbols`
 * distinct characters in all: the shape of the reference's fixture HDFS_2k_multichar.log and of the data set its
 * published numbers are quoted on (> 1,000 distinct symbols, README.md:291-292) */
int fmx_synth_log_multichar(uint64_t seed, int32_t n, int32_t symbols, uint16_t *out);
int fmx_synth_patterns(uint64_t seed, const uint16_t *text, int32_t n, int32_t m, int32_t count, uint16_t *pat,
                       int32_t *pat_off, int32_t *positions);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H */
