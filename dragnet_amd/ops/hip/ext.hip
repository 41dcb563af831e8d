// dragnet_amd MI355X scan engine — torch extension entry point.
//
// Single translation unit: includes the gfx950 kernels and exposes the
// host launchers to Python.  All per-scan device state lives in a
// ScanState: given the uploaded plan buffers and the table sizes it
// allocates, owns and grows the tables, dictionaries and counters its
// descriptors point at, so their layout is stated here alone; the
// per-launch methods take only what changes from launch to launch.  The
// Python engine (dragnet_amd/engine/gpu.py) keeps one per scan context.

#include <torch/extension.h>
#include <cstdlib>
#include <cstring>
#include <c10/hip/HIPStream.h>

#include "scan_kernels.hip"

namespace dn {

namespace {

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU")

constexpr size_t LDS_MAX = 160 * 1024;

hipStream_t current_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// Every kernel launch goes through here (grid, block, dynamic LDS on
// the current stream) so none can skip the launch-error check.
template <class... KArgs, class... Args>
void launch(const char* what, void (*kernel)(KArgs...), dim3 grid,
            dim3 block, size_t lds, Args&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, current_stream(),
                     std::forward<Args>(args)...);
  hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, what, " launch failed: ",
              hipGetErrorString(err));
}

// Largest grid of a scan launch; a dense table has one partial row per
// workgroup, so this is its row count as well.
constexpr uint32_t GRID_CAP = 2048;

uint32_t grid_for(uint64_t n) {
  return (uint32_t)std::min<uint64_t>((n + BLOCK - 1) / BLOCK, GRID_CAP);
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// Dynamic LDS of one launch; the staging tile (if any) comes on top.
size_t lds_bytes(int64_t nf, int64_t nm, int64_t ns, bool columnar) {
  return LdsLayout((int)nf, (int)nm, columnar ? 0 : (int)ns, !columnar)
      .total;
}

using ScanKernel = void (*)(ScanArgs);

// DRAGNET_MIN_WAVES -> linear kernel (2-6 compiled; anything else runs
// the unconstrained build)
ScanKernel linear_kernel(int mw) {
  switch (mw) {
    case 2: return scan_kernel_mw<2>;
    case 3: return scan_kernel_mw<3>;
    case 4: return scan_kernel_mw<4>;
    case 5: return scan_kernel_mw<5>;
    case 6: return scan_kernel_mw<6>;
    default: return scan_kernel;
  }
}

// (DRAGNET_MIN_WAVES, DRAGNET_XGRAN) -> wave-transposed kernel.  r2
// sweep on the device-built layout: 64B granules fastest (1457-1462 vs
// 1436 (32B) vs 1400 (128B) M rec/s); the other granules exist at 4
// waves only.
ScanKernel xpose_kernel(int mw, int xg) {
  if (xg == 32) return scan_kernel_x<4, 5>;
  if (xg == 128) return scan_kernel_x<4, 7>;
  switch (mw) {
    case 2: return scan_kernel_x<2, 6>;
    case 3: return scan_kernel_x<3, 6>;
    case 5: return scan_kernel_x<5, 6>;
    default: return scan_kernel_x<4, 6>;
  }
}

}  // namespace

// Index newlines in a device buffer: fills pos_out (up to its
// capacity) with sorted newline positions and total_out[0] with the
// true count — entirely device-side, no host sync.
void newline_index(torch::Tensor data, int64_t start, int64_t n,
                   torch::Tensor seg_scratch,
                   torch::Tensor pos_out, torch::Tensor total_out) {
  CHECK_GPU(data);
  int64_t span = n - (start & ~(int64_t)15);
  uint32_t nseg = (uint32_t)((span + NL_SEG - 1) / NL_SEG);
  TORCH_CHECK((int64_t)nseg <= seg_scratch.numel(),
              "seg_scratch too small");
  if (span <= 0) {
    total_out.zero_();
    return;
  }
  const uint8_t* d = (const uint8_t*)data.data_ptr();
  uint32_t* segs = (uint32_t*)seg_scratch.data_ptr();
  // wave-per-segment kernels: 256-thread blocks cover 4 segments each
  uint32_t blocks = (nseg + 3) / 4;
  launch("newline_count", newline_count_kernel, dim3(blocks), dim3(256), 0,
         d, (uint32_t)start, (uint32_t)n, segs, nseg);
  launch("newline_scan", newline_scan_kernel, dim3(1), dim3(1024), 0,
         segs, nseg, (uint32_t*)total_out.data_ptr());
  launch("newline_write", newline_write_kernel, dim3(blocks), dim3(256), 0,
         d, (uint32_t)start, (uint32_t)n, segs, nseg,
         (uint32_t*)pos_out.data_ptr(), (uint32_t)pos_out.numel());
}

// Columnar index-query (K7): build the per-slot column descriptor
// array (CPU bytes; caller copies to GPU).  Kinds as scan_columns.h
// has them; a dictionary-coded column passes its codes as soffs[f].
torch::Tensor col_descs_host(std::vector<int64_t> kinds,
                             std::vector<torch::Tensor> nums,
                             std::vector<torch::Tensor> soffs,
                             std::vector<torch::Tensor> slens) {
  int nf = (int)kinds.size();
  auto out = torch::zeros({(long)(nf * sizeof(ColDesc))},
                          torch::dtype(torch::kUInt8));
  ColDesc* d = (ColDesc*)out.data_ptr();
  for (int f = 0; f < nf; f++) {
    d[f].kind = (int32_t)kinds[f];
    d[f].num = kinds[f] == COL_NUM ? (const double*)nums[f].data_ptr()
                                   : nullptr;
    d[f].soff = (kinds[f] == COL_STR || kinds[f] == COL_CODED)
                    ? (const uint32_t*)soffs[f].data_ptr()
                    : nullptr;
    d[f].slen = kinds[f] == COL_STR ? (const uint32_t*)slens[f].data_ptr()
                                    : nullptr;
  }
  return out;
}

// Device-side wave-transpose: scatter length-sorted records into the
// granule-interleaved layout (see xpose_build_kernel).
void xpose_build(torch::Tensor data, torch::Tensor sstart,
                 torch::Tensor slen, torch::Tensor wbase,
                 int64_t n_slots, int64_t gran_log, torch::Tensor xb) {
  CHECK_GPU(data);
  CHECK_GPU(xb);
  uint32_t nw = (uint32_t)(n_slots >> 6);
  TORCH_CHECK(wbase.numel() >= (long)nw + 1, "wbase needs nw+1 rows");
  uint32_t blocks = (nw + 3) / 4;  // 4 waves per 256-thread block
  launch("xpose_build", xpose_build_kernel, dim3(blocks), dim3(256), 0,
         (const uint8_t*)data.data_ptr(),
         (const uint32_t*)sstart.data_ptr(),
         (const uint32_t*)slen.data_ptr(),
         (const unsigned long long*)wbase.data_ptr(),
         (uint32_t)n_slots, (int)gran_log, (uint8_t*)xb.data_ptr());
}

// The bound state of one scan context.  Built once from keyword
// arguments; allocates and owns every tensor its PlanView / AggTable /
// StrDict / NumDict descriptors point at, so their lifetime does not
// depend on what Python happens to keep.  scan* and reset do no
// allocation, host sync or environment read — they are safe inside a
// graph capture.
class ScanState {
 public:
  // plan:  the compiled plan's device buffers and scalars by name; the
  //        state lives on their device
  // agg_slots: of each metric's table; dict_slots: of either dictionary
  // dense: also a [GRID_CAP, agg_slots] f64 partial matrix per metric —
  //        enables dense accumulation + the MFMA reduce
  ScanState(py::dict plan, int64_t agg_slots, int64_t dict_slots,
            int64_t dict_data_bytes, bool dense)
      : dense_(dense) {
    auto ptr = [&](py::dict& d, const char* key) {
      owned_.push_back(py::cast<torch::Tensor>(d[key]));
      return owned_.back().data_ptr();
    };
    PlanView& P = args_.P;
    // the ONE place a PlanView is filled (column_plan adjusts a copy)
    P.field_sigs = (const uint64_t*)ptr(plan, "field_sigs");
    P.nf = (int)owned_.back().numel();
    P.comp_slot = (const int32_t*)ptr(plan, "comp_slot");
    P.nf_match = py::cast<int>(plan["nf_match"]);
    P.sig_bloom = (uint64_t)py::cast<int64_t>(plan["sig_bloom"]);
    P.prog_nodes = (const int32_t*)ptr(plan, "prog_nodes");
    P.prog_bounds = (const int32_t*)ptr(plan, "prog_bounds");
    P.const_meta = (const int32_t*)ptr(plan, "const_meta");
    P.const_dvals = (const double*)ptr(plan, "const_dvals");
    P.const_bytes = (const uint8_t*)ptr(plan, "const_bytes");
    P.synth_slots = (const int32_t*)ptr(plan, "synth_slots");
    P.ns = py::cast<int>(plan["n_synth"]);
    P.metric_rows = (const int32_t*)ptr(plan, "metric_rows");
    P.nm = (int)(owned_.back().numel() / 8);
    P.synth_req = (const int32_t*)ptr(plan, "synth_req");
    P.bd_rows = (const int32_t*)ptr(plan, "bd_rows");
    P.bd_steps = (const double*)ptr(plan, "bd_steps");
    P.value_slot = py::cast<int>(plan["value_slot"]);
    P.fields_slot = py::cast<int>(plan["fields_slot"]);
    P.fields_parent_sig =
        (uint64_t)py::cast<int64_t>(plan["fields_parent_sig"]);
    args_.data_format_skinner = py::cast<bool>(plan["skinner"]) ? 1 : 0;

    // every plan descriptor holds a raw device pointer
    for (auto& t : owned_) CHECK_GPU(t);
    device_ = owned_.front().device();

    // tables, dictionaries and counters: every tensor is a member
    // (reset, extract_all and grow_* use the tensors themselves)
    check_slots(agg_slots, "agg table", AGG_LOG2);
    check_slots(dict_slots, "sdict", DICT_LOG2);
    check_bytes(dict_data_bytes);
    states_.resize(P.nm);
    keys_.resize(P.nm);
    counts_.resize(P.nm);
    if (dense_) partials_.resize(P.nm);
    for (int m = 0; m < P.nm; m++) alloc_agg(m, agg_slots);
    alloc_sdict(dict_slots);
    alloc_ndict(dict_slots);
    sd_data_ = zeros({dict_data_bytes}, U8);
    sd_used_ = zeros({1}, I32);
    sd_next_ = zeros({1}, I32);
    nd_next_ = zeros({1}, I32);
    counters_ = zeros({C_GLOBAL_N + P.nm * CM_N}, I64);
    bind_tables();
    bind_dicts();
    args_.counters = (unsigned long long*)counters_.data_ptr();

    // experiment knobs: read once, here — never per launch.  Default 4
    // waves/SIMD: the parse kernel is latency-bound and the
    // register-allocator cap measured +17% over the unconstrained build
    int mw = env_int("DRAGNET_MIN_WAVES", 4);
    linear_ = linear_kernel(mw);
    xpose_ = xpose_kernel(mw, env_int("DRAGNET_XGRAN", 64));

    lds_ = lds_bytes(P.nf, P.nm, P.ns, false);
    TORCH_CHECK(lds_ <= LDS_MAX, "plan needs too much LDS: ", lds_);
    // optional LDS staging tile (parse from LDS); DRAGNET_LDS_STAGE:
    // 0 = off, -1 = auto (all remaining LDS), >0 = requested bytes.
    // Measured on MI355X: staging costs more occupancy than the
    // global-gather it saves for ~226B records — default off.
    int tile_req = env_int("DRAGNET_LDS_STAGE", 0);
    if (tile_req != 0) {
      size_t avail = (LDS_MAX - lds_ - 256) & ~(size_t)15;
      tile_cap_ = (tile_req < 0) ? avail
                                 : std::min((size_t)tile_req, avail);
      if (tile_cap_ > 100 * 1024) tile_cap_ = 100 * 1024;
      if (tile_cap_ < 24 * 1024) tile_cap_ = 0;
    }
    args_.tile_cap = (uint32_t)tile_cap_;
  }

  // Fused NDJSON scan over one chunk.  The line count lives on-device:
  // launch a full grid and grid-stride.
  void scan(torch::Tensor data, torch::Tensor nl_pos,
            torch::Tensor nlines, int64_t first_start) {
    CHECK_GPU(data);
    CHECK_GPU(nl_pos);
    ScanArgs A = args_;
    A.data = (const uint8_t*)data.data_ptr();
    A.nl_pos = (const uint32_t*)nl_pos.data_ptr();
    A.nlines_ptr = (const uint32_t*)nlines.data_ptr();
    A.pos_cap = (uint32_t)nl_pos.numel();
    A.first_start = (uint32_t)first_start;
    launch("scan_kernel", linear_, dim3(grid_for(A.pos_cap)), dim3(BLOCK),
           lds_ + tile_cap_, A);
  }

  // One scan pass over a wave-transposed staging (scan_kernel_x).
  void scan_xpose(torch::Tensor xdata, torch::Tensor wave_base,
                  torch::Tensor rec_len, int64_t n_slots) {
    CHECK_GPU(xdata);
    TORCH_CHECK(n_slots > 0, "empty transposed staging");
    ScanArgs A = args_;
    A.xdata = (const uint8_t*)xdata.data_ptr();
    A.xwave_base = (const unsigned long long*)wave_base.data_ptr();
    A.xrec_len = (const uint32_t*)rec_len.data_ptr();
    A.xn_slots = (uint32_t)n_slots;
    launch("scan_kernel_x", xpose_, dim3(grid_for(A.xn_slots)),
           dim3(BLOCK), lds_ + tile_cap_, A);
  }

  // Columnar index-query (K7) over uploaded index columns.  col_descs
  // (col_descs_host, on device) holds raw pointers into `columns`; the
  // state keeps every input referenced until its next columnar or coded
  // call, so none can be freed before the launch is enqueued.
  void columnar_query(torch::Tensor col_descs, torch::Tensor blob,
                      torch::Tensor values, int64_t nrows,
                      std::vector<torch::Tensor> columns) {
    ColumnLaunch L = bind_columns("columnar", col_descs, blob, values,
                                  nrows, std::move(columns));
    if (L.blocks == 0) return;
    launch("columnar_query", columnar_query_kernel, dim3(L.blocks),
           dim3(BLOCK), L.lds, L.A);
  }

  // Dictionary-coded index query over the merged sidecar columns of a
  // launch group: interns the launch dictionary (dict_blob, doff, dlen)
  // into the state's StrDict, then evaluates the query over every row,
  // on the current stream.  col_descs holds kinds 0, 1 and 3; seg_start
  // is uint32 [nfiles + 1] row offsets, and the plan's last breakdown is
  // the reserved file column.  The caller has validated codes < ndict
  // and every doff + dlen within dict_blob.
  void coded_query(torch::Tensor col_descs, torch::Tensor dict_blob,
                   torch::Tensor doff, torch::Tensor dlen,
                   torch::Tensor seg_start, torch::Tensor values,
                   int64_t nrows, std::vector<torch::Tensor> columns) {
    for (auto* t : {&doff, &dlen, &seg_start}) CHECK_GPU(*t);
    TORCH_CHECK(doff.numel() == dlen.numel(), "doff / dlen differ");
    TORCH_CHECK(doff.numel() < (int64_t)0xFFFFFFFFll, "dictionary too big");
    TORCH_CHECK(seg_start.numel() >= 2 &&
                    seg_start.numel() - 1 < (int64_t)ORD_BIAS,
                "seg_start needs nfiles + 1 entries");
    ColumnLaunch L = bind_columns("coded", col_descs, dict_blob, values,
                                  nrows, std::move(columns));
    auto code2id = zeros({std::max<int64_t>(doff.numel(), 1)}, I32);
    col_inputs_.insert(col_inputs_.end(),
                       {doff, dlen, seg_start, code2id});
    CodedArgs X;
    X.ndict = (uint32_t)doff.numel();
    X.nfiles = (uint32_t)(seg_start.numel() - 1);
    X.doff = (const uint32_t*)doff.data_ptr();
    X.dlen = (const uint32_t*)dlen.data_ptr();
    X.code2id = (const uint32_t*)code2id.data_ptr();
    X.seg_start = (const uint32_t*)seg_start.data_ptr();
    if (X.ndict > 0)
      launch("dict_intern", dict_intern_kernel,
             dim3((X.ndict + 255) / 256), dim3(256), 0, L.A.sdict, L.A.blob,
             X.doff, X.dlen, X.ndict, (uint32_t*)code2id.data_ptr(),
             overflow_ptr());
    if (L.blocks == 0) return;
    launch("coded_query", coded_query_kernel, dim3(L.blocks), dim3(BLOCK),
           L.lds, L.A, X);
  }

  // One-call zeroing of all scan state: a streaming step otherwise
  // issues ~10 separate torch .zero_() dispatches whose python+dispatch
  // overhead shows at 5 ms/step.
  void reset() {
    hipStream_t st = current_stream();
    auto z = [&](torch::Tensor& t) {
      hipError_t e = hipMemsetAsync(t.data_ptr(), 0,
                                    (size_t)t.numel() * t.element_size(),
                                    st);
      TORCH_CHECK(e == hipSuccess, "reset memset failed: ",
                  hipGetErrorString(e));
    };
    for (auto& t : states_) z(t);
    for (auto& t : counts_) z(t);
    for (auto& t : partials_) z(t);
    z(sd_state_); z(sd_used_); z(sd_next_);
    z(nd_state_); z(nd_next_); z(counters_);
  }

  // One-call snapshot + extraction for the pipelined finalize
  // (gpu._ScanContext.extract_async): clones of the counters and
  // dictionary cursors/blob, the dictionary extractions, and the
  // no-sync per-metric aggregate extraction, enqueued on the current
  // stream in one binding call instead of ~10 python dispatches.
  // aggs is a list of (keys, counts, n) per metric; its buffers are
  // full-capacity and the caller slices by n after its own sync.
  py::dict extract_all() {
    // dense mode: fold the per-workgroup partial matrices into count[]
    // (MFMA column-sum) before the table extraction below reads them
    for (const AggTable& T : tables_) dense_reduce(T);
    const StrDict& sd = args_.sdict;
    const NumDict& nd = args_.ndict;
    py::dict out;
    out["cnt"] = counters_.clone();
    out["n_str"] = sd_next_.clone();
    out["n_num"] = nd_next_.clone();
    out["used"] = sd_used_.clone();
    // the dictionary byte blob is bump-allocated from 0 each scan, so
    // the NEXT step overwrites it — snapshot now
    out["blob"] = sd_data_.clone();

    long n_sids = std::max<long>(sd.nslots, 1);
    auto str_off = zeros({n_sids}, I32);
    auto str_len = zeros({n_sids}, I32);
    if (sd.nslots > 0)
      launch("extract_strdict", extract_strdict_kernel,
             dim3((sd.nslots + 255) / 256), dim3(256), 0, sd,
             (uint32_t*)str_off.data_ptr(), (uint32_t*)str_len.data_ptr(),
             sd.nslots);
    out["str_off"] = str_off;
    out["str_len"] = str_len;

    auto numbers = zeros({std::max<long>(nd.nslots, 1)}, F64);
    if (nd.nslots > 0)
      launch("extract_numdict", extract_numdict_kernel,
             dim3((nd.nslots + 255) / 256), dim3(256), 0, nd,
             (double*)numbers.data_ptr(), nd.nslots);
    out["numbers"] = numbers;

    py::list aggs;
    for (const AggTable& T : tables_) {
      long max_out = T.nslots;
      auto out_keys = zeros({max_out, (long)MAX_KEY}, I32);
      auto out_counts = zeros({max_out}, F64);
      auto out_n = zeros({1}, I32);
      launch("extract_agg", extract_agg_kernel,
             dim3((T.nslots + 255) / 256), dim3(256), 0, T,
             (uint32_t*)out_keys.data_ptr(),
             (double*)out_counts.data_ptr(), (uint32_t*)out_n.data_ptr(),
             (uint32_t)max_out);
      aggs.append(py::make_tuple(out_keys, out_counts, out_n));
    }
    out["aggs"] = aggs;
    return out;
  }

  // Slots / bytes by name, as capacity.CapacityPlanner.names has them.
  py::dict sizes() const {
    py::dict out;
    for (size_t m = 0; m < tables_.size(); m++)
      out[py::str("agg" + std::to_string(m))] = tables_[m].nslots;
    out["sdict"] = args_.sdict.nslots;
    out["sdata"] = args_.sdict.data_cap;
    out["ndict"] = args_.ndict.nslots;
    return out;
  }

  torch::Tensor counters() const { return counters_; }

  // ---- in-place growth (hash path only; engine/capacity.py plans it) ----
  // Each grow_* validates the new size (a rejected call changes
  // nothing), allocates zeroed tensors of that size, rebinds the
  // descriptors and enqueues the rehash (scan_rehash.h) on the current
  // stream; the old tensors stay referenced until that launch is
  // enqueued and are then dropped (the allocator reuses them in stream
  // order).  lds_, the launch knobs and the counters are unaffected: a
  // placement that cannot be made bumps C_OVERFLOW, nothing else does.

  // Current occupancy of every growable structure, on device, no sync:
  // int64 [ready slots per metric..., string ids, payload bytes used,
  // number ids].
  torch::Tensor occupancy() {
    std::vector<torch::Tensor> parts;
    for (auto& st : states_)
      parts.push_back(st.eq((int64_t)SLOT_READY).sum().reshape({1}));
    for (auto* t : {&sd_next_, &sd_used_, &nd_next_})
      parts.push_back(t->to(torch::kInt64));
    return torch::cat(parts);
  }

  void grow_agg(int64_t m, int64_t new_slots) {
    TORCH_CHECK(!dense_, "dense tables do not grow");
    TORCH_CHECK(m >= 0 && (size_t)m < tables_.size(), "no such metric");
    AggTable old = tables_[m];
    check_slots(new_slots, "agg table", AGG_LOG2, old.nslots);
    std::vector<torch::Tensor> keep = {states_[m], keys_[m], counts_[m]};
    growing("agg" + std::to_string(m), old.nslots, new_slots,
            [&] { alloc_agg(m, new_slots); });
    bind_tables();
    launch("rehash_agg", rehash_agg_kernel, dim3((old.nslots + 255) / 256),
           dim3(256), 0, old, tables_[m], overflow_ptr());
  }

  void grow_sdict(int64_t new_slots) {
    StrDict old = args_.sdict;
    check_slots(new_slots, "sdict", DICT_LOG2, old.nslots);
    std::vector<torch::Tensor> keep = {sd_state_, sd_hash_, sd_id_,
                                       sd_off_, sd_len_};
    growing("sdict", old.nslots, new_slots, [&] { alloc_sdict(new_slots); });
    bind_dicts();
    launch("rehash_strdict", rehash_strdict_kernel,
           dim3((old.nslots + 255) / 256), dim3(256), 0, old, args_.sdict,
           overflow_ptr());
  }

  // The payload blob moves to the same offsets: a plain device copy.
  void grow_sdata(int64_t new_bytes) {
    torch::Tensor old = sd_data_;
    check_bytes(new_bytes, old.numel());
    growing("sdata", old.numel(), new_bytes,
            [&] { sd_data_ = zeros({new_bytes}, U8); });
    bind_dicts();
    hipError_t e = hipMemcpyAsync(
        sd_data_.data_ptr(), old.data_ptr(), (size_t)old.numel(),
        hipMemcpyDeviceToDevice, current_stream());
    TORCH_CHECK(e == hipSuccess, "payload copy failed: ",
                hipGetErrorString(e));
  }

  void grow_ndict(int64_t new_slots) {
    NumDict old = args_.ndict;
    check_slots(new_slots, "ndict", DICT_LOG2, old.nslots);
    std::vector<torch::Tensor> keep = {nd_state_, nd_bits_, nd_id_};
    growing("ndict", old.nslots, new_slots, [&] { alloc_ndict(new_slots); });
    bind_dicts();
    launch("rehash_numdict", rehash_numdict_kernel,
           dim3((old.nslots + 255) / 256), dim3(256), 0, old, args_.ndict,
           overflow_ptr());
  }

 private:
  static constexpr auto I32 = torch::kInt32, I64 = torch::kInt64,
                        F64 = torch::kFloat64, U8 = torch::kUInt8;

  torch::Tensor zeros(at::IntArrayRef shape, torch::ScalarType dtype) const {
    return torch::zeros(shape, torch::dtype(dtype).device(device_));
  }

  // A requested slot count: a mask (power of two), uint32 on the device
  // (AGG_LOG2: an aggregation table's keys are indexed slot * MAX_KEY in
  // uint32), and more than the present count where a table grows.
  static constexpr int DICT_LOG2 = 31, AGG_LOG2 = 29;
  static void check_slots(int64_t n, const char* what, int max_log2,
                          int64_t old = 0) {
    TORCH_CHECK(n > 0 && (n & (n - 1)) == 0 && (n >> max_log2) <= 1, what,
                ": slot count must be a power of two <= 2^", max_log2);
    TORCH_CHECK(n > old, "a table may only grow (", old, " -> ", n,
                " slots)");
  }

  // offsets into the payload are uint32
  static void check_bytes(int64_t n, int64_t old = -1) {
    TORCH_CHECK(n <= (int64_t)0xFFFFFFFFll,
                "string payload buffer exceeds 32-bit offsets");
    TORCH_CHECK(n > old, "string payload buffer may only grow");
  }

  // Run one structure's allocation for a growth; a failed device
  // allocation has changed no member and is reported as a RuntimeError.
  template <class Alloc>
  static void growing(const std::string& name, int64_t old_size,
                      int64_t new_size, Alloc&& alloc) {
    try {
      alloc();
    } catch (const c10::OutOfMemoryError& e) {
      std::string why = e.what_without_backtrace();
      TORCH_CHECK(false, "cannot grow ", name, " from ", old_size, " to ",
                  new_size, ": device allocation failed (",
                  why.substr(0, why.find('\n')), ")");
    }
  }

  struct ColumnLaunch {
    ColArgs A;
    size_t lds;
    uint32_t blocks;  // 0: no rows, nothing to launch
  };

  // What a column-query launch (scan_columns.h) takes whichever kernel
  // runs it: checks the inputs against nrows and the plan, keeps them
  // referenced in col_inputs_, and fills the arguments from args_.
  ColumnLaunch bind_columns(const char* what, torch::Tensor col_descs,
                            torch::Tensor blob, torch::Tensor values,
                            int64_t nrows,
                            std::vector<torch::Tensor> columns) {
    for (auto* t : {&col_descs, &blob, &values}) CHECK_GPU(*t);
    for (auto& t : columns) {
      CHECK_GPU(t);
      TORCH_CHECK(t.numel() >= nrows, "column shorter than nrows");
    }
    TORCH_CHECK(nrows >= 0 && nrows < (int64_t)0xFFFFFFFFll, what,
                " query: row count exceeds 32 bits");
    TORCH_CHECK(values.numel() >= nrows, "values shorter than nrows");
    ColumnLaunch L;
    ColArgs& A = L.A;
    A.P = column_plan();
    TORCH_CHECK(col_descs.numel() == (int64_t)(A.P.nf * sizeof(ColDesc)),
                "col_descs does not match the plan's field count");
    L.lds = lds_bytes(A.P.nf, A.P.nm, 0, true);
    TORCH_CHECK(L.lds <= LDS_MAX, what, " plan needs too much LDS");
    A.nrows = (uint32_t)nrows;
    A.values = (const double*)values.data_ptr();
    A.blob = (const uint8_t*)blob.data_ptr();
    A.cols = (const ColDesc*)col_descs.data_ptr();
    A.tables = args_.tables;
    A.sdict = args_.sdict;
    A.ndict = args_.ndict;
    A.counters = args_.counters;
    col_inputs_ = std::move(columns);
    col_inputs_.insert(col_inputs_.end(), {col_descs, blob, values});
    L.blocks = grid_for((uint64_t)nrows);
    return L;
  }

  // The plan as the column kernels see it: columns are pre-extracted,
  // so there are no key sigs and no synthetics.
  PlanView column_plan() const {
    PlanView P = args_.P;
    P.sig_bloom = 0;
    P.fields_parent_sig = 0;
    P.ns = 0;
    P.value_slot = -1;
    P.fields_slot = -1;
    return P;
  }

  unsigned long long* overflow_ptr() {
    return (unsigned long long*)counters_.data_ptr() + C_OVERFLOW;
  }

  // alloc_*: one structure's zeroed tensors at a checked size.  The
  // right-hand side allocates them all before the first member changes.
  void alloc_agg(size_t m, int64_t n) {
    std::tie(states_[m], keys_[m], counts_[m]) = std::make_tuple(
        zeros({n}, I32), zeros({n * MAX_KEY}, I32), zeros({n}, F64));
    if (dense_) partials_[m] = zeros({GRID_CAP, n}, F64);
  }

  void alloc_sdict(int64_t n) {
    std::tie(sd_state_, sd_hash_, sd_id_, sd_off_, sd_len_) =
        std::make_tuple(zeros({n}, I32), zeros({n}, I64), zeros({n}, I32),
                        zeros({n}, I32), zeros({n}, I32));
  }

  void alloc_ndict(int64_t n) {
    std::tie(nd_state_, nd_bits_, nd_id_) =
        std::make_tuple(zeros({n}, I32), zeros({n}, I64), zeros({n}, I32));
  }

  // (Re)build the dictionary descriptors from their tensors.
  void bind_dicts() {
    StrDict& sd = args_.sdict;
    sd.state = (uint32_t*)sd_state_.data_ptr();
    sd.hash = (uint64_t*)sd_hash_.data_ptr();
    sd.id = (uint32_t*)sd_id_.data_ptr();
    sd.off = (uint32_t*)sd_off_.data_ptr();
    sd.len = (uint32_t*)sd_len_.data_ptr();
    sd.nslots = (uint32_t)sd_state_.numel();
    sd.data = (uint8_t*)sd_data_.data_ptr();
    sd.data_cap = (uint32_t)sd_data_.numel();
    sd.data_used = (uint32_t*)sd_used_.data_ptr();
    sd.next_id = (uint32_t*)sd_next_.data_ptr();
    NumDict& nd = args_.ndict;
    nd.state = (uint32_t*)nd_state_.data_ptr();
    nd.bits = (uint64_t*)nd_bits_.data_ptr();
    nd.id = (uint32_t*)nd_id_.data_ptr();
    nd.nslots = (uint32_t)nd_state_.numel();
    nd.next_id = (uint32_t*)nd_next_.data_ptr();
  }

  // (Re)build the per-metric table descriptors from states_/keys_/
  // counts_/partials_ and upload them.
  void bind_tables() {
    size_t nm = states_.size();
    tables_.resize(nm);
    for (size_t m = 0; m < nm; m++) {
      AggTable& t = tables_[m];
      t.state = (uint32_t*)states_[m].data_ptr();
      t.keys = (uint32_t*)keys_[m].data_ptr();
      t.count = (double*)counts_[m].data_ptr();
      t.nslots = (uint32_t)states_[m].numel();
      t.partial = dense_ ? (double*)partials_[m].data_ptr() : nullptr;
      t.prows = dense_ ? GRID_CAP : 0;
      t.pad_ = 0;
    }
    auto host = torch::empty({(long)(nm * sizeof(AggTable))},
                             torch::dtype(torch::kUInt8));
    memcpy(host.data_ptr(), tables_.data(), nm * sizeof(AggTable));
    table_descs_ = host.to(device_);
    args_.tables = (AggTable*)table_descs_.data_ptr();
  }

  // Fold a dense partial matrix into count[] with the MFMA column-sum
  // reduce (must run before extraction of a dense-mode table).
  static void dense_reduce(const AggTable& T) {
    if (T.partial == nullptr || T.prows == 0) return;
    uint32_t tiles = (T.nslots + 15) / 16;
    uint32_t splits = 32;
    while (splits > 1 && T.prows / splits < 16) splits /= 2;
    uint32_t rows_per_blk = (T.prows + splits - 1) / splits;
    rows_per_blk = (rows_per_blk + 3) & ~3u;  // multiple of the K=4 step
    launch("mfma_reduce", mfma_reduce_kernel, dim3(tiles, splits),
           dim3(64), 0, T, rows_per_blk);
  }

  // owned tensors: named where a method needs the tensor itself (or
  // growth replaces it), owned_ for the plan's, which only the
  // descriptors point at
  std::vector<torch::Tensor> states_, keys_, counts_, partials_, owned_;
  std::vector<torch::Tensor> col_inputs_;  // last columnar / coded inputs
  torch::Tensor sd_state_, sd_hash_, sd_id_, sd_off_, sd_len_;
  torch::Tensor sd_data_, sd_used_, sd_next_;
  torch::Tensor nd_state_, nd_bits_, nd_id_, nd_next_;
  torch::Tensor counters_, table_descs_;
  c10::Device device_ = c10::kCPU;  // of the plan tensors
  const bool dense_;
  // prebuilt launch arguments: the PlanView, StrDict and NumDict, the
  // table/counter pointers and the tile size; a launch copies them and
  // sets only its own input fields
  ScanArgs args_ = {};
  std::vector<AggTable> tables_;  // host copy of table_descs_
  // launch configuration cached at construction
  ScanKernel linear_ = nullptr, xpose_ = nullptr;
  size_t lds_ = 0, tile_cap_ = 0;
};

}  // namespace dn

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "dragnet_amd MI355X scan engine (gfx950 HIP kernels)";
  m.def("newline_index", &dn::newline_index, "device-side newline index");
  m.def("xpose_build", &dn::xpose_build, "device-side wave transpose");
  m.def("col_descs_host", &dn::col_descs_host);
  m.def("lds_bytes", &dn::lds_bytes, py::arg("nf"), py::arg("nm"),
        py::arg("ns") = 0, py::arg("columnar") = false,
        "dynamic LDS bytes of a scan / columnar launch (host only)");
  py::class_<dn::ScanState>(m, "ScanState")
      .def(py::init<py::dict, int64_t, int64_t, int64_t, bool>(),
           py::kw_only(), py::arg("plan"), py::arg("agg_slots"),
           py::arg("dict_slots"), py::arg("dict_data_bytes"),
           py::arg("dense"))
      .def("scan", &dn::ScanState::scan, py::arg("data"),
           py::arg("nl_pos"), py::arg("nlines"), py::arg("first_start"),
           "fused NDJSON scan over one chunk")
      .def("scan_xpose", &dn::ScanState::scan_xpose, py::arg("xdata"),
           py::arg("wave_base"), py::arg("rec_len"), py::arg("n_slots"))
      .def("columnar_query", &dn::ScanState::columnar_query,
           py::arg("col_descs"), py::arg("blob"), py::arg("values"),
           py::arg("nrows"), py::arg("columns"),
           "K7: query over uploaded index columns")
      .def("coded_query", &dn::ScanState::coded_query,
           py::arg("col_descs"), py::arg("dict_blob"), py::arg("doff"),
           py::arg("dlen"), py::arg("seg_start"), py::arg("values"),
           py::arg("nrows"), py::arg("keep"),
           "query over merged dictionary-coded sidecar columns")
      .def("reset", &dn::ScanState::reset)
      .def("extract_all", &dn::ScanState::extract_all)
      .def("occupancy", &dn::ScanState::occupancy,
           "device int64 [ready slots per metric..., string ids, "
           "payload bytes, number ids]")
      .def("sizes", &dn::ScanState::sizes)
      .def_property_readonly("counters", &dn::ScanState::counters)
      .def("grow_agg", &dn::ScanState::grow_agg, py::arg("metric"),
           py::arg("new_slots"),
           "rehash one metric's table into a larger zeroed one")
      .def("grow_sdict", &dn::ScanState::grow_sdict, py::arg("new_slots"))
      .def("grow_sdata", &dn::ScanState::grow_sdata, py::arg("new_bytes"))
      .def("grow_ndict", &dn::ScanState::grow_ndict, py::arg("new_slots"));
  m.attr("MAX_KEY") = (int)dn::MAX_KEY;
  m.attr("MAX_FIELDS") = (int)dn::MAX_FIELDS;
}
