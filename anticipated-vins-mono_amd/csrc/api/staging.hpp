// api/staging.hpp - how the arrays travel: stage / on_device, alloc_out / copy_back / scatter over the tables, array_in / array_out / array_back for an array beside a struct

namespace {
constexpr size_t PACK_LIMIT = 4u << 20;  // batches up to 4 MiB (a few windows: the real-time use) travel packed
inline size_t pack_up(size_t n) { return (n + 63) & ~size_t(63); }

// one host array into the pool buffer `name`; a null or empty array gives a null device pointer
int stage_array(avm_ctx* c, const char* name, const void* host, size_t bytes, const void** dev) {
  *dev = nullptr;
  if (!host || bytes == 0) return AVM_OK;
  void* d = pool_get(c, name, bytes);
  if (!d) return fail(c, AVM_ERR_HIP, "hipMalloc failed (staging)");
  HIPCHK(c, hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = d;
  return AVM_OK;
}

// Copies the tables of the host struct *h that entry point `use` reads to the device and points *d (a copy of *h) at them.  pack: the pool
// name of the one block - 64-byte aligned parts, in table order, absent tables left out - that the batch travels in when all of it fits
// PACK_LIMIT: one pinned buffer and one copy (22 pageable copies of a few hundred bytes each cost more than the solve's pre-integration
// kernel); nullptr: table by table, each into the pool buffer of its name (behind `prefix`: a call that stages two structs of one kind).
// dims: the struct the sizes come from (null: *h itself).
int stage(avm_ctx* c, Table t, unsigned use, const void* h, void* d, const char* pack, bool* packed, const char* prefix = "", const void* dims = nullptr) {
  if (!dims) dims = h;
  size_t total = 0;
  for (const Field& f : t)
    if ((f.in & use) && get_ptr(h, f)) total += pack_up(f.bytes(h, dims));
  const bool pk = pack && total <= PACK_LIMIT;
  if (packed) *packed = pk;
  if (!pk) {
    for (const Field& f : t) {
      if (!(f.in & use)) continue;
      const void* dev;
      const int rc = stage_array(c, (std::string(prefix) + f.pool).c_str(), get_ptr(h, f), f.bytes(h, dims), &dev);
      if (rc != AVM_OK) return rc;
      set_ptr(d, f, dev);
    }
    return AVM_OK;
  }
  char* hp = static_cast<char*>(pool_get(c, pack, total, PINNED));
  char* dp = static_cast<char*>(pool_get(c, pack, total));
  if (!hp || !dp) return fail(c, AVM_ERR_HIP, "allocation failed (packed staging)");
  size_t off = 0;
  for (const Field& f : t) {
    const void* host = get_ptr(h, f);
    if (!(f.in & use) || !host) continue;
    std::memcpy(hp + off, host, f.bytes(h, dims));
    set_ptr(d, f, dp + off);
    off += pack_up(f.bytes(h, dims));
  }
  HIPCHK(c, hipMemcpyAsync(dp, hp, total, hipMemcpyHostToDevice, c->stream));
  return AVM_OK;
}

// The caller's struct as the kernels take it: the struct itself (AVM_MEM_DEVICE), or staged (AVM_MEM_HOST).  The entry points that take
// a subset of the window tables never pack.
template <class S>
int on_device(avm_ctx* c, avm_mem mem, Table t, unsigned use, const S* h, S* d, const char* pack = nullptr, bool* packed = nullptr,
              const char* prefix = "", const void* dims = nullptr) {
  *d = *h;
  if (packed) *packed = false;
  return mem == AVM_MEM_HOST ? stage(c, t, use, h, d, pack, packed, prefix, dims) : AVM_OK;
}

// the whole window batch: packed when it is small and has its four state arrays, the head of the block
int windows_on_device(avm_ctx* c, avm_mem mem, const avm_window_batch* h, avm_window_batch* d, bool* packed = nullptr) {
  const bool states = h->pose && h->speedbias && h->ex_pose && h->inv_depth;
  return on_device(c, mem, WINDOWS, U_WHOLE, h, d, states ? "w_pack" : nullptr, packed);
}

// AVM_MEM_HOST: device arrays for the outputs the caller asked for (the non-null members of *h) in *d, a copy of *h - as parts of one
// block `pack` (its size to *pack_bytes), or each under its own pool name
int alloc_out(avm_ctx* c, Table t, const void* h, void* d, const void* dims, const char* pack = nullptr, size_t* pack_bytes = nullptr) {
  size_t total = 0;
  for (const Field& f : t)
    if (get_ptr(h, f)) total += pack_up(f.bytes(h, dims));
  char* block = pack ? static_cast<char*>(pool_get(c, pack, total)) : nullptr;
  if (pack && !block) return AVM_ERR_HIP;
  if (pack) *pack_bytes = total;
  size_t off = 0;
  for (const Field& f : t) {
    void* dev = nullptr;
    if (get_ptr(h, f)) {
      dev = pack ? block + off : pool_get(c, f.pool, f.bytes(h, dims));
      if (!dev) return AVM_ERR_HIP;
      off += pack_up(f.bytes(h, dims));
    }
    set_ptr(d, f, dev);
  }
  return AVM_OK;
}

// what copy_back left in pinned memory for scatter
struct PackedBack {
  const char* pinned = nullptr;
  int n = 0;
};

// AVM_MEM_HOST: the arrays entry point `use` returns, device -> host, enqueued behind the kernels.  The first n_packed of them are the
// head of one packed block on the device: one copy takes them to the pinned buffer `pin`, and scatter() hands them out after the
// synchronize.  The others go straight into the caller's arrays.
int copy_back(avm_ctx* c, avm_mem mem, Table t, unsigned use, const void* h, const void* d, const void* dims, int n_packed = 0,
              const char* pin = nullptr, PackedBack* back = nullptr) {
  if (mem != AVM_MEM_HOST) return AVM_OK;
  int k = 0;
  size_t bytes = 0;
  const void* head = nullptr;
  for (const Field& f : t) {
    void* host = get_ptr(h, f);
    if (!(f.out & use) || !host) continue;
    const void* dev = get_ptr(d, f);
    if (k++ < n_packed) {
      if (!head) head = dev;
      bytes += pack_up(f.bytes(h, dims));
      if (k < n_packed) continue;
      char* hp = static_cast<char*>(pool_get(c, pin, bytes, PINNED));
      if (!hp) return fail(c, AVM_ERR_HIP, "allocation failed (packed copy back)");
      HIPCHK(c, hipMemcpyAsync(hp, head, bytes, hipMemcpyDeviceToHost, c->stream));
      back->pinned = hp, back->n = n_packed;
    } else if (dev) {
      HIPCHK(c, hipMemcpyAsync(host, dev, f.bytes(h, dims), hipMemcpyDeviceToHost, c->stream));
    }
  }
  return AVM_OK;
}

// after the synchronize: the packed arrays into the caller's own
void scatter(Table t, unsigned use, const void* h, const void* dims, const PackedBack& back) {
  int k = 0;
  size_t off = 0;
  for (const Field& f : t) {
    void* host = get_ptr(h, f);
    if (!(f.out & use) || !host) continue;
    if (k++ == back.n) break;
    std::memcpy(host, back.pinned + off, f.bytes(h, dims));
    off += pack_up(f.bytes(h, dims));
  }
}

// an array beside the structs, in `mem` space: the caller's pointer, or (AVM_MEM_HOST) a staged copy / a device buffer to copy back from
template <class T>
int array_in(avm_ctx* c, avm_mem mem, const char* pool, const T* p, size_t n, const T** d) {
  *d = p;
  if (mem != AVM_MEM_HOST) return AVM_OK;
  const void* dev = nullptr;
  const int rc = stage_array(c, pool, p, sizeof(T) * n, &dev);
  *d = static_cast<const T*>(dev);
  return rc;
}
// (an array the call rewrites in place: it travels in, array_back returns it)
template <class T>
int array_inout(avm_ctx* c, avm_mem mem, const char* pool, T* p, size_t n, T** d) {
  const T* in;
  const int rc = array_in(c, mem, pool, static_cast<const T*>(p), n, &in);
  *d = const_cast<T*>(in);
  return rc;
}
// (what: the outputs' name in the message of a failed allocation)
template <class T>
int array_out(avm_ctx* c, avm_mem mem, const char* pool, T* p, size_t n, T** d, const char* what = "output array") {
  *d = p;
  if (mem != AVM_MEM_HOST || !p) return AVM_OK;
  *d = static_cast<T*>(pool_get(c, pool, sizeof(T) * n));
  if (!*d) c->err = std::string("hipMalloc failed (") + what + ")";
  return *d ? AVM_OK : AVM_ERR_HIP;
}
template <class T>
int array_back(avm_ctx* c, avm_mem mem, T* p, const T* d, size_t n) {
  if (mem == AVM_MEM_HOST && p && d && n) HIPCHK(c, hipMemcpyAsync(p, d, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
  return AVM_OK;
}
// a result the ctx holds on the device, into the caller's array in `mem` space (null: not asked for)
template <class T>
int array_from_ctx(avm_ctx* c, avm_mem mem, T* p, const T* src, size_t n) {
  if (p) HIPCHK(c, hipMemcpyAsync(p, src, sizeof(T) * n, mem == AVM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
  return AVM_OK;
}
}  // namespace
