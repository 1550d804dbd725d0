// Probe of the engine's scan, compaction, adjacency and fill primitives (tests/test_gpu_primitives.py).
//
//   primitives_probe DIR
//
// reads DIR/manifest.txt -- one case per line, `name kind key=value ...` -- and the raw little-endian arrays
// DIR/<name>.<tag>.bin, runs every case on the engine's stream through the internal cfx:: functions of
// libcutfemx_amd.so (the compact* templates of cfx_device.h are instantiated here) and writes the raw results to
// DIR/<name>.<tag>.out and one line of numbers per case (per pass of a step) to DIR/results.txt.  It generates
// nothing and checks nothing: both stay in Python.  A case that throws cfx::Error is named on stderr and in
// results.txt with the message, and the probe exits with status 2 without running the cases behind it.
#include "../../cutfemx_amd/csrc/cfx_common.h"
#include "../../cutfemx_amd/csrc/cfx_device.h"

#include <fstream>
#include <sstream>

using namespace cfx;

namespace
{
std::string g_dir;
FILE* g_results = nullptr;

struct Case
{
  std::string name, kind;
  std::map<std::string, std::string> kv;
  std::string str(const char* key) const
  {
    auto it = kv.find(key);
    if (it == kv.end()) throw Error(CFX_ERR_INVALID_ARGUMENT, std::string("manifest: missing ") + key);
    return it->second;
  }
  int64_t num(const char* key) const { return atoll(str(key).c_str()); }
  std::string path(const std::string& tag, const char* ext) const { return g_dir + "/" + name + "." + tag + ext; }
};

template <typename T>
std::vector<T> read_file(const std::string& path, int64_t n)
{
  std::vector<T> v((size_t)n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw Error(CFX_ERR_INVALID_ARGUMENT, "cannot open " + path);
  const size_t got = n > 0 ? fread(v.data(), sizeof(T), (size_t)n, f) : 0;
  const bool at_end = fgetc(f) == EOF;
  fclose(f);
  if (got != (size_t)n || !at_end) throw Error(CFX_ERR_INVALID_ARGUMENT, "wrong size: " + path);
  return v;
}

template <typename T>
void write_file(const std::string& path, const std::vector<T>& v)
{
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) throw Error(CFX_ERR_RUNTIME, "cannot write " + path);
  const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
  if (fclose(f) != 0 || put != v.size()) throw Error(CFX_ERR_RUNTIME, "short write: " + path);
}

void sync() { CFX_HIP(hipStreamSynchronize(ctx().stream)); }

template <typename T>
void upload(DevArray<T>& d, const std::vector<T>& h)
{
  d.alloc((int64_t)h.size());
  if (!h.empty()) CFX_HIP(hipMemcpy(d.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
}

template <typename T>
std::vector<T> fetch(const T* dev, int64_t n)
{
  sync();
  std::vector<T> h((size_t)n);
  if (n > 0) CFX_HIP(hipMemcpy(h.data(), dev, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost));
  return h;
}

template <typename T>
void poison(DevArray<T>& d, int64_t elements, int byte = 0xa5)
{
  d.alloc(elements);
  if (elements > 0) CFX_HIP(hipMemsetAsync(d.p, byte, sizeof(T) * (size_t)elements, ctx().stream));
}

// ---- scans: out holds n + 2 words, the last one poison that must survive ----
template <typename Tin, typename Tout>
void run_scan(const Case& c)
{
  const int64_t n = c.num("n");
  DevArray<Tin> in;
  upload(in, read_file<Tin>(c.path("in", ".bin"), n));
  DevArray<Tout> out;
  poison(out, n + 2);
  exclusive_scan(in.p, out.p, n);
  write_file(c.path("out", ".out"), fetch(out.p, n + 2));
}

template <typename Tin>
void run_scan_pair(const Case& c)
{
  const int64_t n = c.num("n");
  DevArray<Tin> a, b;
  upload(a, read_file<Tin>(c.path("a", ".bin"), n));
  upload(b, read_file<Tin>(c.path("b", ".bin"), n));
  DevArray<int64_t> oa, ob;
  poison(oa, n + 2);
  poison(ob, n + 2);
  exclusive_scan_pair(a.p, oa.p, b.p, ob.p, n);
  write_file(c.path("outa", ".out"), fetch(oa.p, n + 2));
  write_file(c.path("outb", ".out"), fetch(ob.p, n + 2));
}

// elements of cur[0..m) that differ from first[0..m), added to *diff
template <typename T>
__global__ void __launch_bounds__(kBlock) differ_kernel(const T* __restrict__ first, const T* __restrict__ cur, int64_t m,
                                                        unsigned long long* diff)
{
  unsigned long long d = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock)
    d += first[i] != cur[i] ? 1ull : 0ull;
  if (d) atomicAdd(diff, d);
}

// the same input scanned `count` times (every repetition takes a fresh slice of the state pool); repetitions 1.. go to
// a second buffer, poisoned before each, and are compared on the device with the first output
template <typename Tin, typename Tout, bool Pair>
void run_scan_repeat(const Case& c)
{
  const int64_t n = c.num("n"), count = c.num("count"), m = n + 2;
  DevArray<Tin> a, b;
  upload(a, read_file<Tin>(c.path(Pair ? "a" : "in", ".bin"), n));
  if (Pair) upload(b, read_file<Tin>(c.path("b", ".bin"), n));
  DevArray<Tout> firstA, firstB, curA, curB;
  poison(firstA, m);
  poison(curA, m);
  if (Pair) { poison(firstB, m); poison(curB, m); }
  DevArray<unsigned long long> diffs;
  poison(diffs, count, 0);
  const dim3 grid = grid_for(std::min<int64_t>(m, 1 << 18), kBlock);
  for (int64_t r = 0; r < count; ++r)
  {
    Tout* oa = r == 0 ? firstA.p : curA.p;
    Tout* ob = r == 0 ? firstB.p : curB.p;
    if (r > 0)
    {
      CFX_HIP(hipMemsetAsync(curA.p, 0xa5, sizeof(Tout) * (size_t)m, ctx().stream));
      if (Pair) CFX_HIP(hipMemsetAsync(curB.p, 0xa5, sizeof(Tout) * (size_t)m, ctx().stream));
    }
    if constexpr (Pair) exclusive_scan_pair(a.p, oa, b.p, ob, n);
    else exclusive_scan(a.p, oa, n);
    if (r > 0)
    {
      launch("probe_differ", differ_kernel<Tout>, grid, dim3(kBlock), 0, firstA.p, curA.p, m, diffs.p + r);
      if (Pair) launch("probe_differ", differ_kernel<Tout>, grid, dim3(kBlock), 0, firstB.p, curB.p, m, diffs.p + r);
    }
  }
  write_file(c.path("diffs", ".out"), fetch(diffs.p, count));
  write_file(c.path(Pair ? "outa" : "out", ".out"), fetch(firstA.p, m));
  if (Pair) write_file(c.path("outb", ".out"), fetch(firstB.p, m));
}

// ---- compactions ----
struct MarkSet
{
  const int8_t* m;
  __device__ bool operator()(int64_t i) const { return m[i] != 0; }
};
struct MarkBit
{
  const int8_t* m;
  int bit;
  __device__ bool operator()(int64_t i) const { return (m[i] & bit) != 0; }
};
// the hit's index at the hit's position, in an array of the caller's
struct IndexEmit
{
  int32_t* dst = nullptr;
  __device__ void operator()(int64_t o, int64_t i) const { dst[o] = (int32_t)i; }
};

void run_compact(const Case& c)
{
  const int64_t n = c.num("n");
  DevArray<int8_t> marks;
  upload(marks, read_file<int8_t>(c.path("in", ".bin"), n));
  DevArray<int32_t> out;
  const int64_t total = compact("probe_compact", n, MarkSet{marks.p}, out);
  fprintf(g_results, "%s count %lld\n", c.name.c_str(), (long long)total);
  write_file(c.path("out", ".out"), fetch(out.p, total));
}

template <typename F>
void with_byte_test(const Case& c, F f)
{
  const std::string t = c.str("test");
  if (t == "nonzero") f(ByteNonZero{});
  else if (t == "zero") f(ByteZero{});
  else if (t == "mask") f(DomainMask{(int)c.num("mask")});
  else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown byte test " + t);
}

void run_compact_bytes(const Case& c)
{
  const int64_t n = c.num("n");
  DevArray<uint8_t> bytes;
  upload(bytes, read_file<uint8_t>(c.path("in", ".bin"), n));
  with_byte_test(c, [&](auto test) {
    DevArray<int32_t> out;
    const int64_t total = compact_bytes("probe_compact_bytes", n, bytes.p, test, out);
    fprintf(g_results, "%s count %lld\n", c.name.c_str(), (long long)total);
    write_file(c.path("out", ".out"), fetch(out.p, total));
  });
}

void check_api(int status, const char* what)
{
  if (status != CFX_OK) throw Error(status, std::string(what) + ": " + cfx_last_error());
}

// One compaction per input s0, s1, ...: outside a step (steps=0: the single input s0), or each inside a step of the
// loop `name`, repeated while the step reports redo (cutfemx_amd/step.py) -- the second and later steps of a loop are
// speculative.  `body(k, lists, keep)` runs the compaction of input k, leaves what is to be written in `lists` and the
// arrays behind it in `keep`; what a void pass built is not written.
struct ListOut
{
  std::string tag;
  const int32_t* dev;
  Count count; // entries to write (an emitted array: the count of the list it goes with)
};
template <typename Body>
void run_in_steps(const Case& c, Body body)
{
  const int64_t steps = c.num("steps");
  for (int64_t k = 0; k < std::max<int64_t>(steps, 1); ++k)
    for (int pass = 0;; ++pass)
    {
      if (pass >= 3) throw Error(CFX_ERR_RUNTIME, "the step still does not fit after a sized repeat");
      std::vector<ListOut> lists;
      int redo = 0;
      int64_t published = 0, read_back = 0;
      if (steps > 0) check_api(cfx_step_begin(c.name.c_str()), "cfx_step_begin");
      std::vector<std::shared_ptr<void>> keep;
      bool met_void = false;
      try { body(k, lists, keep); }
      catch (const Error& e)
      {
        // a read-back that met the void state of the step before its end: close the step and repeat it
        if (steps == 0 || e.code != CFX_ERR_STEP_VOID) { if (steps > 0) (void)cfx_step_abort(); throw; }
        met_void = true;
      }
      if (steps > 0) check_api(cfx_step_end(&redo, &published, &read_back), "cfx_step_end");
      if (met_void) { redo = 1; lists.clear(); }
      fprintf(g_results, "%s step %lld pass %d redo %d published %lld read_back %lld", c.name.c_str(), (long long)k, pass, redo,
              (long long)published, (long long)read_back);
      for (const ListOut& l : lists) fprintf(g_results, " %s %lld", l.tag.c_str(), redo ? -1ll : (long long)l.count.value());
      fprintf(g_results, "\n");
      if (!redo)
      {
        for (const ListOut& l : lists)
          if (l.dev)
            write_file(g_dir + "/" + c.name + ".s" + std::to_string(k) + "." + l.tag + ".out", fetch(l.dev, l.count.value()));
        break;
      }
    }
}

template <typename T>
std::shared_ptr<DevArray<T>> kept(std::vector<std::shared_ptr<void>>& keep)
{
  auto a = std::make_shared<DevArray<T>>();
  keep.push_back(a);
  return a;
}

void run_compact_count(const Case& c)
{
  const int64_t n = c.num("n");
  run_in_steps(c, [&](int64_t k, std::vector<ListOut>& lists, std::vector<std::shared_ptr<void>>& keep) {
    auto marks = kept<int8_t>(keep);
    upload(*marks, read_file<int8_t>(c.path("s" + std::to_string(k), ".bin"), n));
    auto out = kept<int32_t>(keep);
    auto emitted = kept<int32_t>(keep);
    IndexEmit emit;
    bool pre_called = false;
    auto pre = [&](int64_t cap) { poison(*emitted, cap, 0xff); emit.dst = emitted->p; pre_called = true; };
    const Count total = compact_count("probe_compact_count", "probe.list", DevN(n), MarkSet{marks->p}, *out, &emit, pre);
    lists.push_back({"list", out->p, total});
    // (pre is called by the single-launch form alone: the three-launch form emits nothing)
    if (pre_called && n > 0) lists.push_back({"emit", emitted->p, total});
  });
}

void run_compact_count_pair(const Case& c)
{
  const int64_t n = c.num("n");
  run_in_steps(c, [&](int64_t k, std::vector<ListOut>& lists, std::vector<std::shared_ptr<void>>& keep) {
    auto marks = kept<int8_t>(keep);
    upload(*marks, read_file<int8_t>(c.path("s" + std::to_string(k), ".bin"), n));
    auto outA = kept<int32_t>(keep), outB = kept<int32_t>(keep), emA = kept<int32_t>(keep), emB = kept<int32_t>(keep);
    IndexEmit ea, eb;
    auto pre = [&](int64_t capA, int64_t capB) {
      poison(*emA, capA, 0xff); ea.dst = emA->p;
      poison(*emB, capB, 0xff); eb.dst = emB->p;
    };
    const char* const sites[2] = {"probe.listA", "probe.listB"};
    Count totals[2];
    compact_count_pair("probe_compact_pair", sites, DevN(n), MarkBit{marks->p, 1}, MarkBit{marks->p, 2}, ea, eb, *outA, *outB,
                       totals, pre);
    lists.push_back({"listA", outA->p, totals[0]});
    lists.push_back({"listB", outB->p, totals[1]});
    lists.push_back({"emitA", emA->p, totals[0]});
    lists.push_back({"emitB", emB->p, totals[1]});
  });
}

void run_compact_bytes_count(const Case& c)
{
  const int64_t n = c.num("n");
  with_byte_test(c, [&](auto test) {
    run_in_steps(c, [&](int64_t k, std::vector<ListOut>& lists, std::vector<std::shared_ptr<void>>& keep) {
      auto bytes = kept<uint8_t>(keep);
      upload(*bytes, read_file<uint8_t>(c.path("s" + std::to_string(k), ".bin"), n));
      auto out = kept<int32_t>(keep);
      const Count total = compact_bytes_count("probe_compact_bytes", "probe.bytes", n, bytes->p, test, *out);
      lists.push_back({"list", out->p, total});
    });
  });
}

// ---- incidence inversion ----
void run_adjacency(const Case& c)
{
  const int64_t ncells = c.num("ncells"), width = c.num("width"), nitems = c.num("nitems");
  DevArray<int32_t> map;
  upload(map, read_file<int32_t>(c.path("in", ".bin"), ncells * width));
  Adjacency adj;
  build_adjacency(map.p, ncells, (int)width, nitems, adj);
  write_file(c.path("offsets", ".out"), fetch(adj.offsets.p, nitems + 1));
  write_file(c.path("cells", ".out"), fetch(adj.cells.p, ncells * width));
}

// ---- dev_fill2: each target sits `pad` + `off` bytes inside a poisoned allocation with `pad` bytes behind it ----
void run_fill2(const Case& c)
{
  const int64_t pad = 64;
  const int64_t size[2] = {c.num("sizea"), c.num("sizeb")}, off[2] = {c.num("offa"), c.num("offb")};
  const int byte[2] = {(int)c.num("bytea"), (int)c.num("byteb")};
  DevArray<uint8_t> block[2];
  for (int s = 0; s < 2; ++s) poison(block[s], pad + off[s] + size[s] + pad);
  dev_fill2(block[0].p + pad + off[0], byte[0], (size_t)size[0], block[1].p + pad + off[1], byte[1], (size_t)size[1]);
  write_file(c.path("a", ".out"), fetch(block[0].p, block[0].n));
  write_file(c.path("b", ".out"), fetch(block[1].p, block[1].n));
}

void run_case(const Case& c)
{
  const std::string type = c.kv.count("type") ? c.kv.at("type") : "";
  if (c.kind == "scan")
  {
    if (type == "i32i64") run_scan<int32_t, int64_t>(c);
    else if (type == "i32i32") run_scan<int32_t, int32_t>(c);
    else if (type == "i64i64") run_scan<int64_t, int64_t>(c);
    else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown scan type " + type);
  }
  else if (c.kind == "scan_pair")
  {
    if (type == "i32i64") run_scan_pair<int32_t>(c);
    else if (type == "i64i64") run_scan_pair<int64_t>(c);
    else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown scan_pair type " + type);
  }
  else if (c.kind == "scan_repeat")
  {
    if (type == "i32i64") run_scan_repeat<int32_t, int64_t, false>(c);
    else if (type == "i32i32") run_scan_repeat<int32_t, int32_t, false>(c);
    else if (type == "i64i64") run_scan_repeat<int64_t, int64_t, false>(c);
    else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown scan type " + type);
  }
  else if (c.kind == "scan_pair_repeat")
  {
    if (type == "i32i64") run_scan_repeat<int32_t, int64_t, true>(c);
    else if (type == "i64i64") run_scan_repeat<int64_t, int64_t, true>(c);
    else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown scan_pair type " + type);
  }
  else if (c.kind == "compact") run_compact(c);
  else if (c.kind == "compact_bytes") run_compact_bytes(c);
  else if (c.kind == "compact_count") run_compact_count(c);
  else if (c.kind == "compact_count_pair") run_compact_count_pair(c);
  else if (c.kind == "compact_bytes_count") run_compact_bytes_count(c);
  else if (c.kind == "adjacency") run_adjacency(c);
  else if (c.kind == "fill2") run_fill2(c);
  else throw Error(CFX_ERR_INVALID_ARGUMENT, "manifest: unknown kind " + c.kind);
  sync();
  CFX_HIP(hipGetLastError());
}
} // namespace

int main(int argc, char** argv)
{
  if (argc != 2) { fprintf(stderr, "usage: primitives_probe DIR\n"); return 64; }
  g_dir = argv[1];
  std::ifstream manifest(g_dir + "/manifest.txt");
  if (!manifest) { fprintf(stderr, "primitives_probe: no manifest in %s\n", g_dir.c_str()); return 64; }
  g_results = fopen((g_dir + "/results.txt").c_str(), "w");
  if (!g_results) { fprintf(stderr, "primitives_probe: cannot write results\n"); return 64; }
  if (cfx_init(0) != CFX_OK) { fprintf(stderr, "primitives_probe: cfx_init: %s\n", cfx_last_error()); return 3; }
  std::string line;
  int status = 0;
  while (status == 0 && std::getline(manifest, line))
  {
    std::istringstream is(line);
    Case c;
    if (!(is >> c.name >> c.kind)) continue;
    std::string tok;
    while (is >> tok)
    {
      const size_t eq = tok.find('=');
      if (eq != std::string::npos) c.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    try { run_case(c); }
    catch (const std::exception& e)
    {
      fprintf(stderr, "primitives_probe: case %s failed: %s\n", c.name.c_str(), e.what());
      fprintf(g_results, "%s ERROR %s\n", c.name.c_str(), e.what());
      status = 2;
    }
    fflush(g_results);
  }
  fclose(g_results);
  return status;
}
