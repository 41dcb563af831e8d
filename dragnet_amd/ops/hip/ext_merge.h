// Host bindings of the merge layer, the step after the multi-GPU gather
// (dragnet_amd/merge.py): sort_rows (sort_rows.h), merge_rows
// (merge_rows.h), unify_strings (unify_strings.h), partition_rows
// (partition_rows.h), encode_table (encode_table.h), render_points
// (render_points.h), rank_strings (rank_strings.h), format_numbers
// (format_numbers.h) and parse_points (parse_points.h), free functions
// that keep nothing between calls.
// Part of ext.hip's translation unit, behind its launch plumbing (launch,
// on_dev, allocating, GRID_CAP).
#pragma once

namespace dn {

namespace {

// An argument of these bindings: a contiguous tensor of this dtype and
// rank on the GPU `dev` (its own device, for a function's first).
void check_arg(const char* fn, const char* name, const torch::Tensor& t,
               torch::ScalarType dtype, int64_t rank, torch::Device dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == dtype &&
                  t.dim() == rank && t.is_contiguous(),
              fn, ": ", name, " must be a contiguous ", dtype, " tensor of "
              "rank ", rank, " on the GPU of the first argument");
}

// Slots of a table for n keys: the next power of two at or above 2n,
// floor 1024, at most 2^31 (> n), the most a uint32 slot addresses.
int64_t table_slots(int64_t n) {
  int64_t slots = 1024;
  while (slots < 2 * n && slots < ((int64_t)1 << 31)) slots *= 2;
  return slots;
}

uint32_t sort_span_grid(int64_t n) {
  return (uint32_t)std::min<int64_t>((n + SORT_BLOCK - 1) / SORT_BLOCK,
                                     GRID_CAP);
}

// The passes of the row sort (sort_rows.h) on the current stream: the
// stable permutation that orders rows [n, w], n >= 2, as int32 [n].
// span_dev is what sort_span_kernel left (AND words, then OR words);
// span_host is the same on the host and is needed only for n >
// SORT_TILE, where the host lists the passes.  Never syncs.
torch::Tensor sort_passes(const long long* rows, int64_t n, int w,
                          const unsigned long long* span_dev,
                          const unsigned long long* span_host,
                          torch::Device dev) {
  const auto i32 = on_dev(dev, torch::kInt32);
  struct Column { int c; int nshift; int shift[8]; };
  Column cols[MERGE_W];
  int ncols = 0;
  if (n > SORT_TILE) {
    for (int c = w - 1; c >= 0; c--) {
      const unsigned long long diff = span_host[w + c] ^ span_host[c];
      Column col = {c, 0, {}};
      for (int b = 0; b < 8; b++)
        if ((diff >> (8 * b)) & 0xffull) col.shift[col.nshift++] = 8 * b;
      if (col.nshift) cols[ncols++] = col;
    }
    if (ncols == 0) return torch::arange(n, i32);
  }
  const int64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  const int64_t total = ntiles * SORT_BINS;
  const int64_t nsums = (total + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor key[2], idx[2], hist, sums;
  allocating([&] {
    idx[0] = torch::empty({n}, i32);
    if (n > SORT_TILE) {
      idx[1] = torch::empty({n}, i32);
      key[0] = torch::empty({n}, on_dev(dev, torch::kInt64));
      key[1] = torch::empty({n}, on_dev(dev, torch::kInt64));
      hist = torch::empty({total}, i32);
      sums = torch::empty({nsums}, i32);
    }
  }, "cannot allocate the sort buffers (two key and two index arrays and "
     "the histograms for ", n, " rows)");
  if (n <= SORT_TILE) {
    launch("sort_small", sort_small_kernel, dim3(1), dim3(SORT_BLOCK), 0,
           rows, (uint32_t)n, w, span_dev, (uint32_t*)idx[0].data_ptr());
    return idx[0];
  }
  sort_key_t* kp[2] = {(sort_key_t*)key[0].data_ptr(),
                       (sort_key_t*)key[1].data_ptr()};
  uint32_t* ip[2] = {(uint32_t*)idx[0].data_ptr(),
                     (uint32_t*)idx[1].data_ptr()};
  uint32_t* hp = (uint32_t*)hist.data_ptr();
  uint32_t* sp = (uint32_t*)sums.data_ptr();
  int cur = 0;
  for (int i = 0; i < ncols; i++) {
    launch("sort_key", sort_key_kernel,
           dim3((uint32_t)((n + SORT_BLOCK - 1) / SORT_BLOCK)),
           dim3(SORT_BLOCK), 0, rows, (uint32_t)n, w, cols[i].c,
           i == 0 ? (const uint32_t*)nullptr : (const uint32_t*)ip[cur],
           kp[cur], ip[cur]);
    for (int j = 0; j < cols[i].nshift; j++) {
      const int shift = cols[i].shift[j];
      launch("sort_hist", sort_hist_kernel, dim3((uint32_t)ntiles),
             dim3(SORT_BLOCK), 0, (const sort_key_t*)kp[cur], (uint32_t)n,
             shift, hp, (uint32_t)ntiles);
      launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
             dim3(SORT_BLOCK), 0, hp, (uint32_t)total, sp);
      launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1),
             dim3(SORT_BLOCK), 0, sp, (uint32_t)nsums);
      launch("sort_scatter", sort_scatter_kernel, dim3((uint32_t)ntiles),
             dim3(SORT_BLOCK), 0, (const sort_key_t*)kp[cur],
             (const uint32_t*)ip[cur], kp[cur ^ 1], ip[cur ^ 1],
             (uint32_t)n, shift, (const uint32_t*)hp, (const uint32_t*)sp,
             (uint32_t)ntiles);
      cur ^= 1;
    }
  }
  return idx[cur];
}

}  // namespace

// The stable permutation that sorts the rows of a contiguous int64
// [n, w] GPU tensor lexicographically, column 0 first, each word as a
// signed int64: np.lexsort(rows.T[::-1]), as int32 [n] (sort_rows.h).
// n < 2 launches nothing; n <= SORT_TILE never syncs; beyond that it
// syncs once, to read which bytes vary, and returns the identity with no
// pass when none does.
torch::Tensor sort_rows(torch::Tensor rows) {
  const auto dev = rows.device();
  check_arg("sort_rows", "rows", rows, torch::kInt64, 2, dev);
  TORCH_CHECK(rows.size(1) >= 1 && rows.size(1) <= MERGE_W,
              "sort_rows: rows must be [n, w] with w in 1..", (int)MERGE_W);
  const int64_t n = rows.size(0);
  const int w = (int)rows.size(1);
  TORCH_CHECK(n < ((int64_t)1 << 31), "sort_rows: n exceeds 2^31 rows");
  if (n < 2) return torch::zeros({n}, on_dev(dev, torch::kInt32));

  c10::DeviceGuard guard(dev);
  auto span = torch::zeros({2 * w}, on_dev(dev, torch::kInt64));
  span.narrow(0, 0, w).fill_(-1);
  const long long* rp = (const long long*)rows.data_ptr();
  unsigned long long* span_p = (unsigned long long*)span.data_ptr();
  launch("sort_span", sort_span_kernel, dim3(sort_span_grid(n)),
         dim3(SORT_BLOCK), 0, rp, (uint32_t)n, (const uint32_t*)nullptr, w,
         span_p);
  if (n <= SORT_TILE) return sort_passes(rp, n, w, span_p, nullptr, dev);
  auto host = span.cpu();  // waits for the span
  return sort_passes(rp, n, w, span_p,
                     (const unsigned long long*)host.data_ptr(), dev);
}

// Group identical rows and sum their values (merge_rows.h): rows is
// int64 [n, nk + 1] (key codes, then the tag pack), vals f64 [n].  With
// seg_start / remap / remap_off the rows come in segments, each with a
// remap table for its string-tagged codes (remap concatenated, the
// tables delimited by remap_off); the three go together.  Returns the g
// distinct rows (any order), their sums, and whether the sums are exact:
// if not they depend on the order of the device's adds, and the caller
// must not use them.  hash_mask narrows the home slots (tests);
// max_blocks > 0 caps the grid.  With sort the rows and sums come back
// in np.unique's order (sort_rows.h): the span kernel runs behind the
// compaction on the device-side count, its words come back in the copy
// that fetches g, and the sort passes are enqueued after it.  Syncs
// once either way, to learn g.
std::tuple<torch::Tensor, torch::Tensor, bool> merge_rows(
    torch::Tensor rows, torch::Tensor vals, int64_t nk,
    c10::optional<torch::Tensor> seg_start,
    c10::optional<torch::Tensor> remap,
    c10::optional<torch::Tensor> remap_off, int64_t hash_mask,
    int64_t max_blocks, bool sort) {
  const auto dev = rows.device();
  TORCH_CHECK(nk >= 1 && nk <= MAX_KEY, "merge_rows: nk must be 1..",
              (int)MAX_KEY);
  const int64_t w = nk + 1;
  check_arg("merge_rows", "rows", rows, torch::kInt64, 2, dev);
  TORCH_CHECK(rows.size(1) == w, "merge_rows: rows must be [n, nk + 1]");
  const int64_t n = rows.size(0);
  check_arg("merge_rows", "vals", vals, torch::kFloat64, 1, dev);
  TORCH_CHECK(vals.size(0) == n, "merge_rows: rows has ", n,
              " rows, vals has ", vals.size(0));
  TORCH_CHECK(n < ((int64_t)1 << 31), "merge_rows: n exceeds 2^31 rows");
  TORCH_CHECK(max_blocks >= 0, "merge_rows: max_blocks is negative");
  const bool segmented = seg_start.has_value();
  TORCH_CHECK(segmented == remap.has_value() &&
                  segmented == remap_off.has_value(),
              "merge_rows: seg_start, remap and remap_off go together");

  const auto i64 = on_dev(dev, torch::kInt64);
  const auto f64 = on_dev(dev, torch::kFloat64);
  MergeArgs A = {};
  torch::Tensor seg_dev, off_dev;
  if (segmented) {
    // the segment structure is a few entries per rank: validated on the
    // host, since the kernel indexes remap through it
    auto seg = seg_start->to(torch::kCPU, torch::kInt64).contiguous();
    auto off = remap_off->to(torch::kCPU, torch::kInt64).contiguous();
    TORCH_CHECK(seg.dim() == 1 && seg.numel() >= 2 &&
                    off.dim() == 1 && off.numel() == seg.numel(),
                "merge_rows: seg_start and remap_off need nseg + 1 "
                "entries each");
    check_arg("merge_rows", "remap", *remap, torch::kInt64, 1, dev);
    const int64_t* sp = seg.data_ptr<int64_t>();
    const int64_t* op = off.data_ptr<int64_t>();
    const int64_t nseg = seg.numel() - 1;
    TORCH_CHECK(sp[0] == 0 && op[0] == 0,
                "merge_rows: seg_start and remap_off start at 0");
    for (int64_t i = 0; i < nseg; i++)
      TORCH_CHECK(sp[i] <= sp[i + 1] && op[i] <= op[i + 1],
                  "merge_rows: seg_start and remap_off must not decrease");
    TORCH_CHECK(sp[nseg] == n, "merge_rows: seg_start ends at ", sp[nseg],
                ", rows has ", n);
    TORCH_CHECK(op[nseg] == remap->numel(), "merge_rows: remap_off ends at ",
                op[nseg], ", remap has ", remap->numel());
    seg_dev = seg.to(torch::kInt32).to(dev);
    off_dev = off.to(dev);
    A.nseg = (uint32_t)nseg;
    A.seg_start = (const uint32_t*)seg_dev.data_ptr();
    A.remap = (const long long*)remap->data_ptr();
    A.remap_off = (const long long*)off_dev.data_ptr();
  }
  if (n == 0)
    return std::make_tuple(torch::empty({0, w}, i64), torch::empty({0}, f64),
                           true);

  c10::DeviceGuard guard(dev);
  // a tile is loaded 16 bytes at a time from the base of rows
  if ((uintptr_t)rows.data_ptr() % 16 != 0) rows = rows.clone();

  const int64_t slots = table_slots(n);
  torch::Tensor state, keys, sum, out_rows, out_sums, meta;
  allocating([&] {
    const auto i32 = on_dev(dev, torch::kInt32);
    state = torch::zeros({slots}, i32);
    keys = torch::zeros({slots * w}, i64);
    sum = torch::zeros({slots}, f64);
    out_rows = torch::empty({n, w}, i64);
    out_sums = torch::empty({n}, f64);
    // g, status; with sort the span behind them: AND words, OR words
    meta = torch::zeros({2 + (sort ? 4 * w : 0)}, i32);
    if (sort) meta.narrow(0, 2, 2 * w).fill_(-1);
  }, "cannot allocate the merge table (", slots, " slots for ", n, " rows)");
  uint32_t* meta_p = (uint32_t*)meta.data_ptr();
  A.rows = (const long long*)rows.data_ptr();
  A.vals = (const double*)vals.data_ptr();
  A.n = (uint32_t)n;
  A.hash_mask = (uint64_t)hash_mask;
  A.T.state = (uint32_t*)state.data_ptr();
  A.T.keys = (long long*)keys.data_ptr();
  A.T.sum = (double*)sum.data_ptr();
  A.T.slots = (uint32_t)slots;
  A.T.w = (int)w;
  A.status = meta_p + 1;

  int64_t blocks = std::min<int64_t>((n + MERGE_TILE - 1) / MERGE_TILE,
                                     GRID_CAP);
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  launch("merge_insert", merge_insert_kernel, dim3((uint32_t)blocks),
         dim3(MERGE_TILE), 0, A);
  launch("merge_compact", merge_compact_kernel,
         dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, A.T,
         (long long*)out_rows.data_ptr(), (double*)out_sums.data_ptr(),
         meta_p, meta_p + 1);
  unsigned long long* span_p = (unsigned long long*)(meta_p + 2);
  if (sort)  // sized for n; reads g on the device and exits beyond it
    launch("sort_span", sort_span_kernel, dim3(sort_span_grid(n)),
           dim3(SORT_BLOCK), 0, (const long long*)out_rows.data_ptr(),
           (uint32_t)n, (const uint32_t*)meta_p, (int)w, span_p);
  auto host = meta.cpu();  // waits for the kernels
  const int64_t g = host.data_ptr<int32_t>()[0];
  const uint32_t status = (uint32_t)host.data_ptr<int32_t>()[1];
  TORCH_CHECK(!(status & MERGE_BAD_CODE),
              "merge_rows: a string-tagged code lies outside its segment's "
              "remap table (seg_start / remap_off do not describe these "
              "rows)");
  TORCH_CHECK(!(status & MERGE_FULL), "merge_rows: merge table full");
  if (sort && g > 1) {
    auto perm = sort_passes(
        (const long long*)out_rows.data_ptr(), g, (int)w, span_p,
        (const unsigned long long*)(host.data_ptr<int32_t>() + 2), dev);
    auto sorted_rows = torch::empty({g, w}, i64);
    auto sorted_sums = torch::empty({g}, f64);
    launch("sort_gather", sort_gather_kernel,
           dim3((uint32_t)((g + MERGE_TILE - 1) / MERGE_TILE)),
           dim3(MERGE_TILE), 0, (const long long*)out_rows.data_ptr(),
           (const double*)out_sums.data_ptr(),
           (const uint32_t*)perm.data_ptr(), (uint32_t)g, (int)w,
           (long long*)sorted_rows.data_ptr(),
           (double*)sorted_sums.data_ptr());
    return std::make_tuple(sorted_rows, sorted_sums,
                           !(status & MERGE_INEXACT));
  }
  return std::make_tuple(out_rows.narrow(0, 0, g), out_sums.narrow(0, 0, g),
                         !(status & MERGE_INEXACT));
}

// Number the distinct byte strings among the spans (start[i], length[i])
// of blob in order of first occurrence (unify_strings.h): remap int64 [n]
// is the id of string i, first int64 [g] the index of the first
// occurrence of id g.  hash_mask narrows the hashes (tests); max_blocks >
// 0 caps the grids of the hash and insert kernels.  n == 0 launches
// nothing.  Syncs once, to learn g and whether every span lay inside the
// blob.
std::tuple<torch::Tensor, torch::Tensor> unify_strings(
    torch::Tensor blob, torch::Tensor start, torch::Tensor length,
    int64_t hash_mask, int64_t max_blocks) {
  const auto dev = blob.device();
  check_arg("unify_strings", "blob", blob, torch::kUInt8, 1, dev);
  check_arg("unify_strings", "start", start, torch::kInt64, 1, dev);
  check_arg("unify_strings", "length", length, torch::kInt64, 1, dev);
  const int64_t n = start.size(0);
  TORCH_CHECK(length.size(0) == n, "unify_strings: start has ", n,
              " entries, length has ", length.size(0));
  TORCH_CHECK(n < ((int64_t)1 << 31), "unify_strings: n exceeds 2^31 spans");
  TORCH_CHECK(max_blocks >= 0, "unify_strings: max_blocks is negative");
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  if (n == 0)
    return std::make_tuple(torch::empty({0}, i64), torch::empty({0}, i64));

  c10::DeviceGuard guard(dev);
  // words and 16-byte units are taken at multiples of 8 and 16 from the
  // base of blob
  if ((uintptr_t)blob.data_ptr() % 16 != 0) blob = blob.clone();

  const int64_t slots = table_slots(n);
  const int64_t n8 = (n + 7) / 8 * 8;
  const int64_t nsums = (n8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor table, hash, slot_of, scan, sums, remap, first, meta;
  allocating([&] {
    table = torch::full({slots}, -1, i32);
    hash = torch::empty({n}, i64);
    slot_of = torch::empty({n}, i32);
    scan = torch::empty({n8}, i32);
    sums = torch::empty({nsums}, i32);
    remap = torch::empty({n}, i64);
    first = torch::empty({n}, i64);
    meta = torch::zeros({2}, i32);  // g, status
  }, "cannot allocate the unify table (", slots, " slots for ", n,
     " strings)");
  uint32_t* meta_p = (uint32_t*)meta.data_ptr();
  UnifyArgs A = {};
  A.blob = (const uint8_t*)blob.data_ptr();
  A.blob_len = blob.numel();
  A.start = (const long long*)start.data_ptr();
  A.length = (const long long*)length.data_ptr();
  A.n = (uint32_t)n;
  A.hash_mask = (uint64_t)hash_mask;
  A.hash = (unsigned long long*)hash.data_ptr();
  A.table = (uint32_t*)table.data_ptr();
  A.slot_mask = (uint32_t)(slots - 1);
  A.slot_of = (uint32_t*)slot_of.data_ptr();
  A.status = meta_p + 1;

  const int64_t tiles = (n + UNIFY_TILE - 1) / UNIFY_TILE;
  int64_t blocks = std::min<int64_t>(tiles, GRID_CAP);
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  const uint32_t* table_p = A.table;
  const uint32_t* slot_p = A.slot_of;
  uint32_t* scan_p = (uint32_t*)scan.data_ptr();
  uint32_t* sums_p = (uint32_t*)sums.data_ptr();
  launch("unify_hash", unify_hash_kernel, dim3((uint32_t)blocks),
         dim3(UNIFY_TILE), 0, A);
  launch("unify_insert", unify_insert_kernel, dim3((uint32_t)blocks),
         dim3(UNIFY_TILE), 0, A);
  launch("unify_flag", unify_flag_kernel,
         dim3((uint32_t)((n8 + UNIFY_TILE - 1) / UNIFY_TILE)),
         dim3(UNIFY_TILE), 0, table_p, slot_p, (uint32_t)n, (uint32_t)n8,
         (const uint32_t*)A.status, scan_p);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
         dim3(SORT_BLOCK), 0, scan_p, (uint32_t)n8, sums_p);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK),
         0, sums_p, (uint32_t)nsums);
  launch("unify_emit", unify_emit_kernel, dim3((uint32_t)tiles),
         dim3(UNIFY_TILE), 0, table_p, slot_p, (uint32_t)n,
         (const uint32_t*)scan_p, (const uint32_t*)sums_p,
         (const uint32_t*)A.status, (long long*)remap.data_ptr(),
         (long long*)first.data_ptr(), meta_p);
  auto host = meta.cpu();  // waits for the kernels
  const int64_t g = host.data_ptr<int32_t>()[0];
  const uint32_t status = (uint32_t)host.data_ptr<int32_t>()[1];
  TORCH_CHECK(!(status & UNIFY_BAD_SPAN),
              "unify_strings: a span lies outside the blob (a negative "
              "start or length, or an end beyond ", blob.numel(), " bytes)");
  TORCH_CHECK(!(status & UNIFY_FULL), "unify_strings: unify table full");
  return std::make_tuple(remap, first.narrow(0, 0, g));
}

// Split rows by destination rank (partition_rows.h): rows is int64 [n,
// nk + 1] (key codes, then the tag pack), vals f64 [n], remap the int64
// table of the string-tagged codes (none: the codes pass through).  Row
// i goes to bin hash(row i) % world, world in 1..PART_MAX_WORLD.  Returns
// wire int64 [n, nk + 2] (remapped codes, tag pack, bits of the value),
// grouped by bin, input order kept within a bin, and counts int64
// [world] on the device.  max_blocks > 0 caps the grids (tests).  n == 0
// launches nothing.  Syncs once, to read the status word.
std::tuple<torch::Tensor, torch::Tensor> partition_rows(
    torch::Tensor rows, torch::Tensor vals, int64_t nk, int64_t world,
    c10::optional<torch::Tensor> remap, int64_t max_blocks) {
  const auto dev = rows.device();
  TORCH_CHECK(nk >= 1 && nk <= MAX_KEY, "partition_rows: nk must be 1..",
              (int)MAX_KEY);
  TORCH_CHECK(world >= 1 && world <= PART_MAX_WORLD,
              "partition_rows: world must be 1..", (int)PART_MAX_WORLD,
              ", got ", world);
  const int64_t w = nk + 1;
  check_arg("partition_rows", "rows", rows, torch::kInt64, 2, dev);
  TORCH_CHECK(rows.size(1) == w, "partition_rows: rows must be [n, nk + 1]");
  const int64_t n = rows.size(0);
  check_arg("partition_rows", "vals", vals, torch::kFloat64, 1, dev);
  TORCH_CHECK(vals.size(0) == n, "partition_rows: rows has ", n,
              " rows, vals has ", vals.size(0));
  TORCH_CHECK(n < ((int64_t)1 << 31), "partition_rows: n exceeds 2^31 rows");
  TORCH_CHECK(max_blocks >= 0, "partition_rows: max_blocks is negative");
  if (remap.has_value())
    check_arg("partition_rows", "remap", *remap, torch::kInt64, 1, dev);
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  if (n == 0)
    return std::make_tuple(torch::empty({0, w + 1}, i64),
                           torch::zeros({world}, i64));

  c10::DeviceGuard guard(dev);
  // a round is loaded 16 bytes at a time from the base of rows
  if ((uintptr_t)rows.data_ptr() % 16 != 0) rows = rows.clone();

  const int64_t ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  const int64_t total = world * ntiles;  // <= 2^8 * 2^20
  const int64_t total8 = (total + 7) / 8 * 8;
  const int64_t nsums = (total8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor wire, counts, hist, sums, status;
  allocating([&] {
    wire = torch::empty({n, w + 1}, i64);
    counts = torch::empty({world}, i64);
    hist = torch::empty({total8}, i32);
    sums = torch::empty({nsums}, i32);
    status = torch::zeros({1}, i32);
  }, "cannot allocate the partition buffers (", n, " wire rows of ", w + 1,
     " words and ", total8, " counts)");
  PartArgs A = {};
  A.rows = (const long long*)rows.data_ptr();
  A.remapped = remap.has_value();
  if (A.remapped) {
    A.remap = (const long long*)remap->data_ptr();
    A.m = remap->numel();
  }
  A.n = (uint32_t)n;
  A.nk = (int)nk;
  A.world = (uint32_t)world;
  while ((1u << A.nbits) < A.world) A.nbits++;
  A.c32 = (uint32_t)(((uint64_t)1 << 32) % (uint64_t)world);

  int64_t blocks = ntiles;
  if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
  uint32_t* hp = (uint32_t*)hist.data_ptr();
  uint32_t* sp = (uint32_t*)sums.data_ptr();
  launch("partition_hist", partition_hist_kernel, dim3((uint32_t)blocks),
         dim3(SORT_BLOCK), 0, A, hp, (uint32_t)ntiles,
         (uint32_t)(total8 - total), (uint32_t*)status.data_ptr());
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
         dim3(SORT_BLOCK), 0, hp, (uint32_t)total8, sp);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK),
         0, sp, (uint32_t)nsums);
  launch("partition_scatter", partition_scatter_kernel,
         dim3((uint32_t)blocks), dim3(SORT_BLOCK), 0, A,
         (const long long*)vals.data_ptr(), (const uint32_t*)hp,
         (const uint32_t*)sp, (uint32_t)ntiles,
         (long long*)wire.data_ptr(), (long long*)counts.data_ptr());
  const uint32_t bits = (uint32_t)status.cpu().data_ptr<int32_t>()[0];
  TORCH_CHECK(!(bits & PART_BAD_CODE),
              "partition_rows: a string-tagged code lies outside the remap "
              "table of ", A.m, " entries");
  return std::make_tuple(wire, counts);
}

// One metric's table of a scan's extraction, to the wire form
// (encode_table.h).  keys int32 [cap, MAX_KEY] (the u32 codes), counts
// f64 [cap], str_off / str_len int32 per string id, blob the payload
// bytes, numbers f64 per number id; n, n_str, used and n_num are int32
// [1] on the device, as the extraction hands them out.  col_kind is per
// breakdown: 0 plain, 1 date, 2 bucketized.  Returns (codes int64 [n,
// nk], tagpack int64 [n], vals f64 [n], dict_blob uint8, dict_offs int64
// [S_dev + 1], exc_kind int32 [E], exc_id int32 [E], exc_blob uint8,
// exc_offs int64 [E + 1], refused): the exceptions have the wire string
// codes S_dev + position and are the caller's to render and append.
// refused: an integer column holds NaN or an infinity, nothing else is
// returned and the host path answers.  Syncs once, after the scans, to
// read the sizes and the status word; the copy and emit kernels are
// enqueued behind that.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, bool>
encode_table(torch::Tensor keys, torch::Tensor counts, torch::Tensor n,
             torch::Tensor str_off, torch::Tensor str_len,
             torch::Tensor n_str, torch::Tensor blob, torch::Tensor used,
             torch::Tensor numbers, torch::Tensor n_num,
             std::vector<int64_t> col_kind) {
  const char* fn = "encode_table";
  const auto dev = keys.device();
  const int64_t nk = (int64_t)col_kind.size();
  TORCH_CHECK(nk >= 1 && nk <= MAX_KEY, fn, ": col_kind needs 1..",
              (int)MAX_KEY, " entries");
  for (int64_t k : col_kind)
    TORCH_CHECK(k >= ENC_COL_PLAIN && k <= ENC_COL_BUCKET, fn,
                ": a column kind is 0 (plain), 1 (date) or 2 (bucketized)");
  check_arg(fn, "keys", keys, torch::kInt32, 2, dev);
  TORCH_CHECK(keys.size(1) == MAX_KEY, fn, ": keys must be [cap, ",
              (int)MAX_KEY, "]");
  const int64_t cap = keys.size(0);
  check_arg(fn, "counts", counts, torch::kFloat64, 1, dev);
  TORCH_CHECK(counts.size(0) == cap, fn, ": keys has ", cap,
              " rows, counts has ", counts.size(0));
  check_arg(fn, "str_off", str_off, torch::kInt32, 1, dev);
  check_arg(fn, "str_len", str_len, torch::kInt32, 1, dev);
  TORCH_CHECK(str_off.size(0) == str_len.size(0), fn,
              ": str_off and str_len differ in length");
  check_arg(fn, "blob", blob, torch::kUInt8, 1, dev);
  check_arg(fn, "numbers", numbers, torch::kFloat64, 1, dev);
  for (auto* t : {&n, &n_str, &used, &n_num}) {
    check_arg(fn, "n / n_str / used / n_num", *t, torch::kInt32, 1, dev);
    TORCH_CHECK(t->numel() == 1, fn, ": n, n_str, used and n_num hold one "
                "int32 each");
  }
  const int64_t str_cap = str_off.size(0), num_cap = numbers.size(0);
  TORCH_CHECK(cap < ((int64_t)1 << 31), fn, ": cap exceeds 2^31 rows");

  // the segments of the one scanned array, each a multiple of 8 long
  const int64_t s8 = (str_cap + 7) / 8 * 8, n8 = (num_cap + 7) / 8 * 8;
  EncArgs A = {};
  int64_t at = 0;
  for (int k = 0; k < ENC_SEGS; k++) {
    A.seg[k] = (uint32_t)at;
    const bool by_number = k == ENC_XNUM_F || k == ENC_XNUM_B ||
                           k == ENC_INT_F || k == ENC_INT_B;
    at += by_number ? n8 : s8;
  }
  A.seg[ENC_SEGS] = (uint32_t)at;
  const int64_t total = at + 8;
  // a segment's own total stays below 2^32: its differences are exact
  TORCH_CHECK(total < ((int64_t)1 << 31) &&
                  2 * blob.numel() + 17 * num_cap + 64 < ((int64_t)1 << 32),
              fn, ": dictionaries too large for 32-bit offsets");
  const int64_t nsums = (total + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;

  c10::DeviceGuard guard(dev);
  // 16-byte loads from the bases of keys and blob
  if ((uintptr_t)keys.data_ptr() % 16 != 0) keys = keys.clone();
  if ((uintptr_t)blob.data_ptr() % 16 != 0) blob = blob.clone();

  const auto u8 = on_dev(dev, torch::kUInt8);
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  torch::Tensor sflags, nflags, scan, sums, meta;
  allocating([&] {
    sflags = torch::zeros({3, std::max<int64_t>(str_cap, 1)}, u8);
    nflags = torch::zeros({2, std::max<int64_t>(num_cap, 1)}, u8);
    scan = torch::zeros({total}, i32);
    sums = torch::empty({nsums}, i32);
    meta = torch::zeros({ENC_M_WORDS}, i32);
  }, "cannot allocate the encode buffers (", total, " scan entries)");
  A.keys = (const uint32_t*)keys.data_ptr();
  A.counts = (const double*)counts.data_ptr();
  A.n_ptr = (const uint32_t*)n.data_ptr();
  A.cap = (uint32_t)cap;
  A.str_off = (const uint32_t*)str_off.data_ptr();
  A.str_len = (const uint32_t*)str_len.data_ptr();
  A.n_str_ptr = (const uint32_t*)n_str.data_ptr();
  A.str_cap = (uint32_t)str_cap;
  A.blob = (const uint8_t*)blob.data_ptr();
  A.used_ptr = (const uint32_t*)used.data_ptr();
  A.blob_cap = (uint32_t)blob.numel();
  A.numbers = (const double*)numbers.data_ptr();
  A.n_num_ptr = (const uint32_t*)n_num.data_ptr();
  A.num_cap = (uint32_t)num_cap;
  A.nk = (int)nk;
  for (int64_t j = 0; j < nk; j++) A.col_kind[j] = (uint8_t)col_kind[j];
  A.str_used = (uint8_t*)sflags[0].data_ptr();
  A.arr_used = (uint8_t*)sflags[1].data_ptr();
  A.str_cls = (uint8_t*)sflags[2].data_ptr();
  A.num_used = (uint8_t*)nflags[0].data_ptr();
  A.num_cls = (uint8_t*)nflags[1].data_ptr();
  A.scan = (uint32_t*)scan.data_ptr();
  A.sums = (uint32_t*)sums.data_ptr();
  A.meta = (uint32_t*)meta.data_ptr();

  auto blocks = [](int64_t items) {
    return (uint32_t)std::max<int64_t>((items + ENC_BLOCK - 1) / ENC_BLOCK, 1);
  };
  const uint32_t str_grid = std::min(blocks(str_cap), GRID_CAP);
  launch("encode_mark", encode_mark_kernel,
         dim3(std::min(blocks(cap), GRID_CAP)), dim3(ENC_BLOCK), 0, A);
  launch("encode_classify", encode_classify_kernel, dim3(str_grid),
         dim3(ENC_BLOCK), 0, A);
  launch("encode_numbers", encode_numbers_kernel, dim3(blocks(num_cap)),
         dim3(ENC_BLOCK), 0, A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
         dim3(SORT_BLOCK), 0, A.scan, (uint32_t)total, A.sums);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK),
         0, A.sums, (uint32_t)nsums);
  launch("encode_totals", encode_totals_kernel, dim3(1), dim3(64), 0, A);
  auto host = meta.cpu();  // waits for the kernels
  const uint32_t* mp = (const uint32_t*)host.data_ptr<int32_t>();
  const uint32_t status = mp[ENC_M_STATUS];
  TORCH_CHECK(!(status & ENC_BAD_TAG), fn, ": a key code has a tag its "
              "column cannot hold (an ordinal outside a bucketized column, "
              "a string or special in one, or an unknown special)");
  TORCH_CHECK(!(status & ENC_BAD_ID), fn, ": a key code names a string or "
              "number id beyond the dictionary (n_str / n_num)");
  TORCH_CHECK(!(status & ENC_BAD_SPAN), fn, ": a referenced string's span "
              "ends beyond the used payload bytes");
  const int64_t rows = mp[ENC_M_N];
  const int64_t sdev = mp[ENC_M_SDEV], E = mp[ENC_M_E];
  torch::Tensor codes, tagpack, vals, dict_blob, dict_offs, exc_kind, exc_id,
      exc_blob, exc_offs;
  if (status & ENC_REFUSED) {
    auto none = torch::empty({0}, i64);
    return std::make_tuple(none, none, none, none, none, none, none, none,
                           none, true);
  }
  allocating([&] {
    codes = torch::empty({rows, nk}, i64);
    tagpack = torch::empty({rows}, i64);
    vals = torch::empty({rows}, on_dev(dev, torch::kFloat64));
    dict_blob = torch::empty({(int64_t)mp[ENC_M_DBYTES]}, u8);
    dict_offs = torch::empty({sdev + 1}, i64);
    exc_kind = torch::empty({E}, i32);
    exc_id = torch::empty({E}, i32);
    exc_blob = torch::empty({(int64_t)mp[ENC_M_EBYTES]}, u8);
    exc_offs = torch::empty({E + 1}, i64);
  }, "cannot allocate the wire table (", rows, " rows, ", sdev + E,
     " strings)");
  A.codes = (long long*)codes.data_ptr();
  A.tagpack = (long long*)tagpack.data_ptr();
  A.vals = (double*)vals.data_ptr();
  A.dict_blob = (uint8_t*)dict_blob.data_ptr();
  A.dict_offs = (long long*)dict_offs.data_ptr();
  A.exc_kind = (int*)exc_kind.data_ptr();
  A.exc_id = (int*)exc_id.data_ptr();
  A.exc_blob = (uint8_t*)exc_blob.data_ptr();
  A.exc_offs = (long long*)exc_offs.data_ptr();
  launch("encode_strings", encode_strings_kernel, dim3(str_grid),
         dim3(ENC_BLOCK), 0, A);
  launch("encode_digits", encode_digits_kernel, dim3(blocks(num_cap)),
         dim3(ENC_BLOCK), 0, A);
  if (rows > 0)
    launch("encode_emit", encode_emit_kernel, dim3(blocks(rows)),
           dim3(ENC_BLOCK), 0, A);
  return std::make_tuple(codes, tagpack, vals, dict_blob, dict_offs, exc_kind,
                         exc_id, exc_blob, exc_offs, false);
}

// The merged table as NDJSON point lines (render_points.h): rows int64
// [g, nk + 1] (key codes, then the tag pack) and sums f64 [g] as
// merge_rows leaves them; order int32 [g] (none: row order), line i being
// row order[i]; dict_blob / dict_offs int64 [G + 1] the global dictionary
// in wire form; col_kind per breakdown 0 plain, 1 date, 2 quantize, 3
// lquantize with col_step its step; seg_blob / seg_offs int64 [nk + 3] the
// nk + 2 constant pieces of a line.  Returns (text uint8
// [bytes], line_off int64 [g + 1], refused).  refused: some element or
// value is one only Python renders (beyond int64, fractional, NaN,
// infinite, F64-tagged) or the dictionary is too large for 32-bit
// offsets; the tensors are empty and the host path answers.  g == 0
// launches nothing.  Syncs once, after the measuring kernels, to read the
// status word and the two byte totals; the escape and emit kernels are
// enqueued behind that.
std::tuple<torch::Tensor, torch::Tensor, bool> render_points(
    torch::Tensor rows, torch::Tensor sums,
    c10::optional<torch::Tensor> order, torch::Tensor dict_blob,
    torch::Tensor dict_offs, std::vector<int64_t> col_kind,
    std::vector<int64_t> col_step, torch::Tensor seg_blob,
    torch::Tensor seg_offs) {
  const char* fn = "render_points";
  const auto dev = rows.device();
  const int64_t nk = (int64_t)col_kind.size();
  TORCH_CHECK(nk >= 1 && nk <= MAX_KEY, fn, ": col_kind needs 1..",
              (int)MAX_KEY, " entries");
  TORCH_CHECK((int64_t)col_step.size() == nk, fn,
              ": col_kind and col_step differ in length");
  for (int64_t k : col_kind)
    TORCH_CHECK(k >= REN_COL_PLAIN && k <= REN_COL_LQUANTIZE, fn,
                ": a column kind is 0 (plain), 1 (date), 2 (quantize) or 3 "
                "(lquantize)");
  check_arg(fn, "rows", rows, torch::kInt64, 2, dev);
  TORCH_CHECK(rows.size(1) == nk + 1, fn, ": rows must be [g, nk + 1]");
  const int64_t g = rows.size(0);
  check_arg(fn, "sums", sums, torch::kFloat64, 1, dev);
  TORCH_CHECK(sums.size(0) == g, fn, ": rows has ", g, " rows, sums has ",
              sums.size(0));
  if (order.has_value()) {
    check_arg(fn, "order", *order, torch::kInt32, 1, dev);
    TORCH_CHECK(order->size(0) == g, fn, ": rows has ", g,
                " rows, order has ", order->size(0));
  }
  check_arg(fn, "dict_blob", dict_blob, torch::kUInt8, 1, dev);
  check_arg(fn, "dict_offs", dict_offs, torch::kInt64, 1, dev);
  TORCH_CHECK(dict_offs.size(0) >= 1, fn, ": dict_offs needs G + 1 entries");
  const int64_t G = dict_offs.size(0) - 1;
  TORCH_CHECK(g < ((int64_t)1 << 31) && G < ((int64_t)1 << 31), fn,
              ": more than 2^31 rows or strings");
  check_arg(fn, "seg_blob", seg_blob, torch::kUInt8, 1, dev);
  check_arg(fn, "seg_offs", seg_offs, torch::kInt64, 1, dev);
  TORCH_CHECK(seg_offs.size(0) == nk + 3 &&
                  seg_blob.numel() < (int64_t)REN_MAX_LINE,
              fn, ": seg_offs needs nk + 3 entries and seg_blob fewer than ",
              REN_MAX_LINE, " bytes");
  RenArgs A = {};
  const auto u8 = on_dev(dev, torch::kUInt8);
  const auto i64 = on_dev(dev, torch::kInt64);
  if (g == 0)
    return std::make_tuple(torch::empty({0}, u8), torch::zeros({1}, i64),
                           false);
  auto none = [&] {
    return std::make_tuple(torch::empty({0}, u8), torch::empty({0}, i64),
                           true);
  };
  // the escaped dictionary is at most this long and is offset in u32
  if (6 * dict_blob.numel() + 2 * G + 64 >= ((int64_t)1 << 32)) return none();

  c10::DeviceGuard guard(dev);
  // 16-byte loads from the base of dict_blob
  if ((uintptr_t)dict_blob.data_ptr() % 16 != 0) dict_blob = dict_blob.clone();

  const int64_t G8 = (G + 1 + 7) / 8 * 8, g8 = (g + 1 + 7) / 8 * 8;
  const int64_t esc_nsums = (G8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  const int64_t line_nsums = (g8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  const auto i32 = on_dev(dev, torch::kInt32);
  torch::Tensor esc_scan, esc_sums, line_scan, line_sums, line_base,
      meta;
  allocating([&] {
    esc_scan = torch::zeros({G8}, i32);
    esc_sums = torch::empty({esc_nsums}, i32);
    line_scan = torch::zeros({g8}, i32);
    line_sums = torch::empty({line_nsums}, i32);
    line_base = torch::empty({line_nsums}, i64);
    meta = torch::zeros({REN_M_WORDS}, i64);
  }, "cannot allocate the render buffers (", G8 + g8, " scan entries)");
  A.rows = (const long long*)rows.data_ptr();
  A.sums = (const double*)sums.data_ptr();
  A.order = order.has_value() ? (const uint32_t*)order->data_ptr() : nullptr;
  A.g = (uint32_t)g;
  A.nk = (int)nk;
  A.dict_blob = (const uint8_t*)dict_blob.data_ptr();
  A.dict_len = dict_blob.numel();
  A.dict_offs = (const long long*)dict_offs.data_ptr();
  A.G = (uint32_t)G;
  for (int64_t j = 0; j < nk; j++) {
    A.col_kind[j] = (uint8_t)col_kind[j];
    A.col_step[j] = (long long)col_step[j];
  }
  A.seg_blob = (const uint8_t*)seg_blob.data_ptr();
  A.seg_len = seg_blob.numel();
  A.seg_offs = (const long long*)seg_offs.data_ptr();
  A.esc_scan = (uint32_t*)esc_scan.data_ptr();
  A.esc_sums = (uint32_t*)esc_sums.data_ptr();
  A.line_scan = (uint32_t*)line_scan.data_ptr();
  A.line_sums = (uint32_t*)line_sums.data_ptr();
  A.line_nsums = (uint32_t)line_nsums;
  A.line_base = (long long*)line_base.data_ptr();
  A.meta = (unsigned long long*)meta.data_ptr();

  auto blocks = [](int64_t items) {
    return dim3((uint32_t)((items + REN_BLOCK - 1) / REN_BLOCK));
  };
  if (G > 0)
    launch("render_escape_measure", render_escape_measure_kernel, blocks(G),
           dim3(REN_BLOCK), 0, A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)esc_nsums),
         dim3(SORT_BLOCK), 0, A.esc_scan, (uint32_t)G8, A.esc_sums);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK), 0,
         A.esc_sums, (uint32_t)esc_nsums);
  launch("render_measure", render_measure_kernel, blocks(g), dim3(REN_BLOCK),
         0, A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)line_nsums),
         dim3(SORT_BLOCK), 0, A.line_scan, (uint32_t)g8, A.line_sums);
  launch("render_totals", render_totals_kernel, dim3(1), dim3(SORT_BLOCK), 0,
         A);
  auto host = meta.cpu();  // waits for the kernels
  const int64_t* mp = host.data_ptr<int64_t>();
  const uint32_t status = (uint32_t)mp[REN_M_STATUS];
  TORCH_CHECK(!(status & REN_BAD_DICT), fn, ": dict_offs does not ascend "
              "from 0 within the ", dict_blob.numel(), " bytes of dict_blob");
  TORCH_CHECK(!(status & REN_BAD_UTF8), fn, ": a dictionary string is "
              "ill-formed UTF-8");
  TORCH_CHECK(!(status & REN_BAD_SEG), fn, ": seg_offs does not ascend from "
              "0 to the ", seg_blob.numel(), " bytes of seg_blob");
  TORCH_CHECK(!(status & REN_BAD_ORDER), fn, ": an order entry lies outside "
              "the ", g, " rows");
  TORCH_CHECK(!(status & REN_BAD_TAG), fn, ": a key element's tag is none of "
              "INT, STR and F64");
  TORCH_CHECK(!(status & REN_BAD_CODE), fn, ": a string-tagged code lies "
              "outside the dictionary of ", G, " strings");
  if (status & REN_REFUSED) return none();
  torch::Tensor esc_blob, text, line_off;
  allocating([&] {
    esc_blob = torch::empty({mp[REN_M_ESC_BYTES]}, u8);
    text = torch::empty({mp[REN_M_TEXT_BYTES]}, u8);
    line_off = torch::empty({g + 1}, i64);
  }, "cannot allocate the point lines (", mp[REN_M_TEXT_BYTES], " bytes for ",
     g, " rows)");
  A.esc_blob = (uint8_t*)esc_blob.data_ptr();
  A.esc_len = esc_blob.numel();
  A.text = (uint8_t*)text.data_ptr();
  A.line_off = (long long*)line_off.data_ptr();
  if (G > 0)
    launch("render_escape", render_escape_kernel, blocks(G), dim3(REN_BLOCK),
           0, A);
  launch("render_emit", render_emit_kernel, blocks(g), dim3(REN_BLOCK), 0, A);
  return std::make_tuple(text, line_off, false);
}

// The rank of every string of a dictionary in byte order
// (rank_strings.h): blob uint8 [bytes], offs int64 [G + 1] ascending from
// 0 within the blob.  Returns (rank int64 [G], duplicate): rank[i] is the
// number of strings smaller than string i, bytes unsigned, a prefix
// first; duplicate: some string occurs twice, the ranks are then
// unspecified and the caller ranks on the host.  finish_max is the
// largest tied group the finish kernel takes (RANK_FINISH_MAX; another
// value is for measurements, 0 never runs it).  G == 0 launches nothing.
// Syncs once in front of each round of 7 string bytes, to read the
// round's active count, the span of its rows and the status word; once
// more when that copy shows the sort over (no string still tied), or,
// where the finish kernel ends it, behind that kernel.
std::tuple<torch::Tensor, bool> rank_strings(torch::Tensor blob,
                                             torch::Tensor offs,
                                             int64_t finish_max) {
  const char* fn = "rank_strings";
  const auto dev = blob.device();
  check_arg(fn, "blob", blob, torch::kUInt8, 1, dev);
  check_arg(fn, "offs", offs, torch::kInt64, 1, dev);
  TORCH_CHECK(offs.size(0) >= 1, fn, ": offs needs G + 1 entries");
  const int64_t G = offs.size(0) - 1;
  TORCH_CHECK(G < ((int64_t)1 << 31) - 16, fn, ": more than 2^31 strings");
  TORCH_CHECK(finish_max >= 0, fn, ": finish_max is negative");
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  if (G == 0) return std::make_tuple(torch::empty({0}, i64), false);

  c10::DeviceGuard guard(dev);
  // aligned 8-byte words from the base of blob, the last one whole
  const int64_t bytes = blob.numel();
  if ((uintptr_t)blob.data_ptr() % 16 != 0 || bytes % 8 != 0) {
    auto padded = torch::empty({(bytes + 7) / 8 * 8},
                               on_dev(dev, torch::kUInt8));
    padded.narrow(0, 0, bytes).copy_(blob);
    blob = padded;
  }

  const int64_t G8 = (G + 1 + 7) / 8 * 8;
  const int64_t nsums = (2 * G8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor rank, rows, scan, sums, sid, headpos, act[2], grp[2],
      gstart[2], meta;
  allocating([&] {
    rank = torch::empty({G}, i64);
    rows = torch::empty({G, 2}, i64);
    scan = torch::empty({2 * G8}, i32);
    sums = torch::empty({nsums}, i32);
    sid = torch::empty({G}, i32);
    headpos = torch::empty({G + 1}, i32);
    for (int k = 0; k < 2; k++) {
      act[k] = torch::empty({G}, i32);
      grp[k] = torch::empty({G}, i32);
      gstart[k] = torch::empty({G}, i32);
    }
    meta = torch::zeros({RANK_M_WORDS}, i64);
    meta.narrow(0, RANK_M_SPAN, 2).fill_(-1);
    meta.narrow(0, RANK_M_COUNT, 1).fill_(G);
  }, "cannot allocate the rank buffers (", G, " strings)");
  const uint64_t* words = (const uint64_t*)blob.data_ptr();
  const long long* offs_p = (const long long*)offs.data_ptr();
  long long* rows_p = (long long*)rows.data_ptr();
  uint32_t* scan_p = (uint32_t*)scan.data_ptr();
  uint32_t* sums_p = (uint32_t*)sums.data_ptr();
  uint32_t* sid_p = (uint32_t*)sid.data_ptr();
  uint32_t* head_p = (uint32_t*)headpos.data_ptr();
  unsigned long long* meta_p = (unsigned long long*)meta.data_ptr();
  auto u32 = [](torch::Tensor& t) { return (uint32_t*)t.data_ptr(); };
  auto blocks = [](int64_t items) {
    return dim3((uint32_t)((items + RANK_BLOCK - 1) / RANK_BLOCK));
  };
  // the rows of the active list `cur` (none: round 0) at `depth`, at most
  // cap of them, and the bytes of theirs that vary
  auto keys_and_span = [&](int cur, int64_t cap, int64_t depth) {
    launch("rank_key", rank_key_kernel, blocks(cap), dim3(RANK_BLOCK), 0,
           words, (long long)bytes, offs_p,
           cur < 0 ? (const uint32_t*)nullptr : (const uint32_t*)u32(act[cur]),
           cur < 0 ? (const uint32_t*)nullptr : (const uint32_t*)u32(grp[cur]),
           (uint32_t)cap, (long long)depth, (longlong2*)rows_p, meta_p);
    launch("sort_span", sort_span_kernel, dim3(sort_span_grid(cap)),
           dim3(SORT_BLOCK), 0, (const long long*)rows_p, (uint32_t)cap,
           (const uint32_t*)(meta_p + RANK_M_COUNT), 2, meta_p + RANK_M_SPAN);
  };

  int cur = -1;  // the active list's buffers; -1: every string, round 0
  int64_t m = G, depth = 0;
  keys_and_span(cur, m, depth);
  for (;;) {
    auto host = meta.cpu();  // waits for the kernels
    const int64_t* mp = host.data_ptr<int64_t>();
    const uint32_t status = (uint32_t)mp[RANK_M_STATUS];
    TORCH_CHECK(!(status & RANK_BAD_DICT), fn, ": offs does not ascend from "
                "0 within the ", bytes, " bytes of blob");
    if (status & RANK_DUPLICATE) return std::make_tuple(rank, true);
    if (cur >= 0) {
      m = mp[RANK_M_COUNT];
      if (m == 0) break;
      if (mp[RANK_M_MAXRUN] <= finish_max) {
        launch("rank_finish", rank_finish_kernel, blocks(m), dim3(RANK_BLOCK),
               0, words, (long long)bytes, offs_p,
               (const uint32_t*)u32(act[cur]), (const uint32_t*)u32(grp[cur]),
               (const uint32_t*)u32(gstart[cur]), (uint32_t)m,
               (long long)depth, (long long*)rank.data_ptr(), meta_p);
        const auto last = meta.cpu();  // waits for the finish
        return std::make_tuple(
            rank, (last.data_ptr<int64_t>()[RANK_M_STATUS] &
                   RANK_DUPLICATE) != 0);
      }
    }
    const int64_t m8 = (m + 1 + 7) / 8 * 8;
    const int64_t round_sums =
        (2 * m8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
    auto perm = m >= 2
        ? sort_passes((const long long*)rows_p, m, 2,
                      meta_p + RANK_M_SPAN,
                      (const unsigned long long*)(mp + RANK_M_SPAN), dev)
        : torch::zeros({1}, i32);
    const int nxt = cur < 0 ? 0 : cur ^ 1;
    const uint32_t* act_p = cur < 0 ? nullptr : u32(act[cur]);
    const uint32_t* grp_p = cur < 0 ? nullptr : u32(grp[cur]);
    const uint32_t* gstart_p = cur < 0 ? nullptr : u32(gstart[cur]);
    launch("rank_bound", rank_bound_kernel, blocks(m8), dim3(RANK_BLOCK), 0,
           (const longlong2*)rows_p, (const uint32_t*)perm.data_ptr(), act_p,
           (uint32_t)m, (uint32_t)m8, scan_p, sid_p, meta_p);
    launch("sort_scan", sort_scan_kernel, dim3((uint32_t)round_sums),
           dim3(SORT_BLOCK), 0, scan_p, (uint32_t)(2 * m8), sums_p);
    launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK),
           0, sums_p, (uint32_t)round_sums);
    launch("rank_heads", rank_heads_kernel, blocks(m), dim3(RANK_BLOCK), 0,
           (const uint32_t*)scan_p, (const uint32_t*)sums_p, (uint32_t)m,
           head_p);
    launch("rank_assign", rank_assign_kernel, blocks(m), dim3(RANK_BLOCK), 0,
           (const uint32_t*)scan_p, (const uint32_t*)sums_p,
           (const uint32_t*)head_p, (const uint32_t*)sid_p, grp_p, gstart_p,
           (uint32_t)m, (uint32_t)m8, (long long*)rank.data_ptr(),
           u32(act[nxt]), u32(grp[nxt]), u32(gstart[nxt]), meta_p);
    cur = nxt;
    depth += RANK_CHUNK;
    keys_and_span(cur, m, depth);
  }
  return std::make_tuple(rank, false);
}

// The JavaScript strings of f64 values (format_numbers.h): x f64 [n].
// Returns (text uint8 [bytes], offs int64 [n + 1]): string i is
// text[offs[i] : offs[i + 1]], ECMAScript Number::toString of x[i], what
// plan.number_key gives.  variant is for measurements (FMT_RECOMPUTE = 1:
// convert in both passes and park nothing; FMT_LDS_TABLE = 2: the power
// table staged in LDS); 0 is what runs.  n == 0 launches nothing.  Syncs
// once, after the measuring kernels, to read the byte total; the emit
// kernel is enqueued behind that.
std::tuple<torch::Tensor, torch::Tensor> format_numbers(torch::Tensor x,
                                                        int64_t variant) {
  const char* fn = "format_numbers";
  const auto dev = x.device();
  check_arg(fn, "x", x, torch::kFloat64, 1, dev);
  const int64_t n = x.size(0);
  TORCH_CHECK(n < ((int64_t)1 << 31) - 16, fn, ": more than 2^31 numbers");
  TORCH_CHECK(variant >= 0 && variant <= 3, fn, ": variant is 0..3");
  const auto u8 = on_dev(dev, torch::kUInt8);
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  if (n == 0)
    return std::make_tuple(torch::empty({0}, u8), torch::zeros({1}, i64));

  c10::DeviceGuard guard(dev);
  const bool parked = !(variant & FMT_RECOMPUTE);
  const int64_t n8 = (n + 1 + 7) / 8 * 8;
  const int64_t nsums = (n8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor dig, form, len_scan, len_sums, base, meta;
  allocating([&] {
    dig = torch::empty({parked ? n : 0}, i64);
    form = torch::empty({parked ? n : 0}, i32);
    len_scan = torch::zeros({n8}, i32);
    len_sums = torch::empty({nsums}, i32);
    base = torch::empty({nsums}, i64);
    meta = torch::zeros({1}, i64);
  }, "cannot allocate the format buffers (", n, " numbers)");
  FmtArgs A = {};
  A.x = (const double*)x.data_ptr();
  A.n = (uint32_t)n;
  A.dig = (unsigned long long*)dig.data_ptr();
  A.form = (uint32_t*)form.data_ptr();
  A.len_scan = (uint32_t*)len_scan.data_ptr();
  A.len_sums = (uint32_t*)len_sums.data_ptr();
  A.nsums = (uint32_t)nsums;
  A.base = (long long*)base.data_ptr();
  A.meta = (unsigned long long*)meta.data_ptr();

  using Kernel = void (*)(FmtArgs);
  static const Kernel measure[4] = {
      format_measure_kernel<0>, format_measure_kernel<1>,
      format_measure_kernel<2>, format_measure_kernel<3>};
  static const Kernel emit[4] = {
      format_emit_kernel<0>, format_emit_kernel<1>, format_emit_kernel<2>,
      format_emit_kernel<3>};
  const dim3 grid((uint32_t)((n + FMT_BLOCK - 1) / FMT_BLOCK));
  launch("format_measure", measure[variant], grid, dim3(FMT_BLOCK), 0, A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
         dim3(SORT_BLOCK), 0, A.len_scan, (uint32_t)n8, A.len_sums);
  launch("format_totals", format_totals_kernel, dim3(1), dim3(SORT_BLOCK), 0,
         A);
  const int64_t bytes = meta.cpu().data_ptr<int64_t>()[0];  // waits
  torch::Tensor text, offs;
  allocating([&] {
    text = torch::empty({bytes}, u8);
    offs = torch::empty({n + 1}, i64);
  }, "cannot allocate the number strings (", bytes, " bytes for ", n,
     " numbers)");
  A.text = (uint8_t*)text.data_ptr();
  A.offs = (long long*)offs.data_ptr();
  launch("format_emit", emit[variant], grid, dim3(FMT_BLOCK), 0, A);
  return std::make_tuple(text, offs);
}

// Tagged point lines to rows (parse_points.h): text uint8 [data_len + 9],
// the NDJSON data and directly behind it the bytes `undefined`; the
// metrics' columns as points.fast_reduce_spec gives them, flattened:
// ncols per metric, then kinds (0 plain, 1 date, 2 quantize, 3 lquantize),
// steps and names over all columns in order, the names as one byte string
// with name_offs [columns + 1].  Returns (metric int32 [t], rows int64
// [t, kmax + 1], span_start int64 [s], span_len int64 [s], vals f64 [t],
// counters int64 [M, 2], punts int64 [p, 2], cls uint8 [lines]): the taken
// lines in line order, kmax the largest column count (unused columns 0,
// the last word the tag pack), a STR element an index into the spans,
// which point into text; per metric ninputs and nonnumeric; the stripped
// byte range of every punted line; the class of every line.  Syncs twice:
// for the line count, and for the three totals that size the outputs.
// An empty text launches nothing.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
parse_points(torch::Tensor text, int64_t data_len,
             std::vector<int64_t> ncols, std::vector<int64_t> kinds,
             std::vector<double> steps, std::string names,
             std::vector<int64_t> name_offs) {
  const char* fn = "parse_points";
  const auto dev = text.device();
  check_arg(fn, "text", text, torch::kUInt8, 1, dev);
  TORCH_CHECK(data_len >= 0 && data_len < ((int64_t)1 << 31) &&
                  text.numel() == data_len + (int64_t)PP_TAIL,
              fn, ": text must hold data_len < 2^31 bytes and the ",
              PP_TAIL, " bytes `undefined` behind them");
  const int64_t M = (int64_t)ncols.size();
  TORCH_CHECK(M >= 1 && M <= PP_MAX_METRICS, fn, ": 1..",
              (int)PP_MAX_METRICS, " metrics");
  const int64_t C = (int64_t)kinds.size();
  TORCH_CHECK((int64_t)steps.size() == C && (int64_t)name_offs.size() == C + 1,
              fn, ": kinds, steps and name_offs (+ 1) differ in length");
  TORCH_CHECK(name_offs[0] == 0 && name_offs[C] == (int64_t)names.size() &&
                  names.size() <= (size_t)PP_NAME_BYTES,
              fn, ": name_offs must run from 0 to the ", names.size(),
              " bytes of names, at most ", (int)PP_NAME_BYTES);
  PpSpecs P;
  memset(&P, 0, sizeof(P));
  P.nm = (int32_t)M;
  memcpy(P.names, names.data(), names.size());
  int kmax = 0;
  int64_t c = 0;
  for (int64_t m = 0; m < M; m++) {
    TORCH_CHECK(ncols[m] >= 0 && ncols[m] <= MAX_KEY && c + ncols[m] <= C, fn,
                ": a metric has 0..", (int)MAX_KEY, " columns");
    P.nk[m] = (uint8_t)ncols[m];
    kmax = std::max(kmax, (int)ncols[m]);
    for (int64_t j = 0; j < ncols[m]; j++, c++) {
      TORCH_CHECK(kinds[c] >= PP_COL_PLAIN && kinds[c] <= PP_COL_LQUANTIZE &&
                      name_offs[c] <= name_offs[c + 1],
                  fn, ": a column kind is 0..3 and name_offs ascends");
      P.kind[m][j] = (uint8_t)kinds[c];
      P.step[m][j] = steps[c];
      P.name_off[m][j] = (uint16_t)name_offs[c];
      P.name_len[m][j] = (uint16_t)(name_offs[c + 1] - name_offs[c]);
    }
  }
  TORCH_CHECK(c == C, fn, ": ncols sums to ", c, ", kinds has ", C);

  const auto u8 = on_dev(dev, torch::kUInt8);
  const auto i32 = on_dev(dev, torch::kInt32);
  const auto i64 = on_dev(dev, torch::kInt64);
  const auto f64 = on_dev(dev, torch::kFloat64);
  auto result = [&](int64_t t, int64_t s, int64_t p, torch::Tensor counters,
                    torch::Tensor cls) {
    return std::make_tuple(
        torch::empty({t}, i32), torch::empty({t, (int64_t)kmax + 1}, i64),
        torch::empty({s}, i64), torch::empty({s}, i64), torch::empty({t}, f64),
        counters, torch::empty({p, 2}, i64), cls);
  };
  if (data_len == 0)
    return result(0, 0, 0, torch::zeros({M, 2}, i64), torch::empty({0}, u8));

  c10::DeviceGuard guard(dev);
  // 16-byte loads from the base of text
  if ((uintptr_t)text.data_ptr() % 16 != 0) text = text.clone();

  PpArgs A = {};
  const int64_t nseg = (data_len + PP_NL_SEG - 1) / PP_NL_SEG;
  const int64_t seg8 = (nseg + 1 + 7) / 8 * 8;
  const int64_t seg_nsums = (seg8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor specs, seg_scan, seg_sums, meta, counters;
  allocating([&] {
    specs = torch::from_blob(&P, {(int64_t)sizeof(P)}, torch::kUInt8).to(dev);
    seg_scan = torch::zeros({seg8}, i32);
    seg_sums = torch::empty({seg_nsums}, i32);
    meta = torch::zeros({PP_M_WORDS}, i64);
    counters = torch::zeros({M, 2}, i64);
  }, "cannot allocate the line index (", seg8, " segments)");
  A.text = (const uint8_t*)text.data_ptr();
  A.data_len = (uint32_t)data_len;
  A.specs = (const PpSpecs*)specs.data_ptr();
  A.kmax = kmax;
  A.nseg = (uint32_t)nseg;
  A.seg_scan = (uint32_t*)seg_scan.data_ptr();
  A.seg_sums = (uint32_t*)seg_sums.data_ptr();
  A.meta = (unsigned long long*)meta.data_ptr();
  A.counters = (unsigned long long*)counters.data_ptr();

  const dim3 seg_grid((uint32_t)((nseg + 3) / 4));
  launch("parse_nl_count", parse_nl_count_kernel, seg_grid, dim3(PP_BLOCK), 0,
         A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)seg_nsums),
         dim3(SORT_BLOCK), 0, A.seg_scan, (uint32_t)seg8, A.seg_sums);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK), 0,
         A.seg_sums, (uint32_t)seg_nsums);
  launch("parse_lines", parse_lines_kernel, dim3(1), dim3(64), 0, A);
  auto host = meta.cpu();  // waits for the kernels
  const int64_t n_nl = host.data_ptr<int64_t>()[PP_M_NL];
  const int64_t n_lines = host.data_ptr<int64_t>()[PP_M_LINES];

  const int64_t n8 = (n_lines + 1 + 7) / 8 * 8;
  const int64_t nsums = (3 * n8 + SORT_SCAN_TILE - 1) / SORT_SCAN_TILE;
  torch::Tensor nl_pos, cls, scan, sums;
  allocating([&] {
    nl_pos = torch::empty({n_nl}, i32);
    cls = torch::empty({n_lines}, u8);
    scan = torch::zeros({3 * n8}, i32);
    sums = torch::empty({nsums}, i32);
  }, "cannot allocate the line buffers (", n_lines, " lines)");
  A.n_nl = (uint32_t)n_nl;
  A.n_lines = (uint32_t)n_lines;
  A.nl_pos = (uint32_t*)nl_pos.data_ptr();
  A.cls = (uint8_t*)cls.data_ptr();
  A.n8 = (uint32_t)n8;
  A.scan = (uint32_t*)scan.data_ptr();
  A.sums = (uint32_t*)sums.data_ptr();
  const dim3 line_grid((uint32_t)((n_lines + PP_BLOCK - 1) / PP_BLOCK));
  if (n_nl > 0)
    launch("parse_nl_write", parse_nl_write_kernel, seg_grid, dim3(PP_BLOCK),
           0, A);
  launch("parse_measure", parse_measure_kernel, line_grid, dim3(PP_BLOCK), 0,
         A);
  launch("parse_measure_global", parse_measure_global_kernel, line_grid,
         dim3(PP_BLOCK), 0, A);
  launch("sort_scan", sort_scan_kernel, dim3((uint32_t)nsums),
         dim3(SORT_BLOCK), 0, A.scan, (uint32_t)(3 * n8), A.sums);
  launch("sort_scan_sums", sort_scan_sums_kernel, dim3(1), dim3(SORT_BLOCK), 0,
         A.sums, (uint32_t)nsums);
  launch("parse_totals", parse_totals_kernel, dim3(1), dim3(64), 0, A);
  host = meta.cpu();  // waits for the kernels
  const int64_t* mp = host.data_ptr<int64_t>();
  decltype(result(0, 0, 0, counters, cls)) out;
  allocating([&] {
    out = result(mp[PP_M_TAKEN], mp[PP_M_SPANS], mp[PP_M_PUNTS], counters,
                 cls);
  }, "cannot allocate the parsed rows (", mp[PP_M_TAKEN], " rows, ",
     mp[PP_M_SPANS], " spans)");
  A.n_taken = (uint32_t)mp[PP_M_TAKEN];
  A.n_spans = (uint32_t)mp[PP_M_SPANS];
  A.n_punts = (uint32_t)mp[PP_M_PUNTS];
  A.metric = (int*)std::get<0>(out).data_ptr();
  A.rows = (long long*)std::get<1>(out).data_ptr();
  A.span_start = (long long*)std::get<2>(out).data_ptr();
  A.span_len = (long long*)std::get<3>(out).data_ptr();
  A.vals = (double*)std::get<4>(out).data_ptr();
  A.punts = (long long*)std::get<6>(out).data_ptr();
  if (A.n_taken || A.n_punts) {
    launch("parse_emit", parse_emit_kernel, line_grid, dim3(PP_BLOCK), 0, A);
    if (mp[PP_M_WIDE])  // some tile did not fit the stage
      launch("parse_emit_global", parse_emit_global_kernel, line_grid,
             dim3(PP_BLOCK), 0, A);
  }
  return out;
}

}  // namespace dn
