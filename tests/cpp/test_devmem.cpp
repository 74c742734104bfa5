// The owning buffer of loik_amd/csrc/loik_devmem.hpp over a counting, malloc-backed policy that can be told to fail its next
// allocation.  Stand-alone (own main, no GPU): tests/test_devmem.py builds it with the address and undefined-behaviour sanitizers,
// so a double free, a leak or a use after free ends the run with a non-zero status whatever the checks below say.
#include "../../loik_amd/csrc/loik_devmem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace {

struct Counting {
  static long live, live_bytes, allocs, frees;
  static bool fail_next;
  static void* last_freed;
  static bool allocate(void** out, size_t bytes)
  {
    ++allocs;
    if (fail_next) { fail_next = false; return false; }
    *out = std::malloc(bytes);
    if (!*out) return false;
    ++live; live_bytes += (long)bytes;
    return true;
  }
  static void free(void* p, size_t bytes)
  {
    ++frees; --live; live_bytes -= (long)bytes;
    last_freed = p;
    std::free(p);
  }
};
long Counting::live = 0, Counting::live_bytes = 0, Counting::allocs = 0, Counting::frees = 0;
bool Counting::fail_next = false;
void* Counting::last_freed = nullptr;

using Buf = loikb::OwnedBuf<Counting, unsigned char>;

int g_failed = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

// what regrow and replace share; `grow` is one of the two
template <class Grow>
void check_growth(Grow grow)
{
  Buf b;
  CHECK(!b && b.bytes() == 0);
  CHECK(grow(b, 0) && !b && Counting::allocs == 0);   // (a zero-byte request of an empty buffer: no call, still empty)
  const long a0 = Counting::allocs, f0 = Counting::frees;
  CHECK(grow(b, 100) && b && b.bytes() == 100 && Counting::allocs == a0 + 1 && Counting::live == 1 && Counting::live_bytes == 100);
  unsigned char* p = b;
  // no larger than what it has: the same pointer, no allocator call
  CHECK(grow(b, 100) && grow(b, 40) && grow(b, 0));
  CHECK((unsigned char*)b == p && b.bytes() == 100 && Counting::allocs == a0 + 1 && Counting::frees == f0);
  // a growth frees the old block exactly once
  CHECK(grow(b, 300) && b.bytes() == 300 && Counting::allocs == a0 + 2 && Counting::frees == f0 + 1 && Counting::last_freed == p);
  CHECK(Counting::live == 1 && Counting::live_bytes == 300);
  CHECK(b.as<int>() == (int*)(unsigned char*)b);
  // release returns the former size and is idempotent
  CHECK(b.release() == 300 && !b && b.bytes() == 0 && Counting::frees == f0 + 2);
  CHECK(b.release() == 0 && Counting::frees == f0 + 2 && Counting::live == 0 && Counting::live_bytes == 0);
}

struct Holder {   // as Chunk / Set of the host layer: a struct of buffers beside plain members, move-only by its members
  int id = 0;
  Buf a, b;
  std::vector<int> scratch;
};

}  // namespace

int main()
{
  check_growth([](Buf& b, size_t n) { return b.regrow(n); });
  Counting::allocs = Counting::frees = 0;
  check_growth([](Buf& b, size_t n) { return b.replace(n); });

  {   // a failed regrow: the old block freed, the buffer empty
    Buf b;
    CHECK(b.regrow(64));
    unsigned char* p = b;
    const long f0 = Counting::frees;
    Counting::fail_next = true;
    CHECK(!b.regrow(128));
    CHECK(!b && b.bytes() == 0 && Counting::frees == f0 + 1 && Counting::last_freed == p && Counting::live == 0 && Counting::live_bytes == 0);
    CHECK(b.regrow(16) && b.bytes() == 16);   // (usable again)
  }
  {   // a failed replace: pointer, size and contents untouched
    Buf b;
    CHECK(b.replace(64));
    unsigned char* p = b;
    std::memset(p, 0xa5, 64);
    const long f0 = Counting::frees;
    Counting::fail_next = true;
    CHECK(!b.replace(128));
    CHECK((unsigned char*)b == p && b.bytes() == 64 && Counting::frees == f0 && Counting::live == 1 && Counting::live_bytes == 64);
    bool same = true;
    for (int i = 0; i < 64; ++i) same = same && p[i] == 0xa5;
    CHECK(same);
    CHECK(b.replace(128) && b.bytes() == 128 && Counting::frees == f0 + 1 && Counting::last_freed == p);
  }
  CHECK(Counting::live == 0 && Counting::live_bytes == 0);

  {   // moves leave the source empty and free nothing twice; swap exchanges
    Buf a;
    CHECK(a.regrow(32));
    unsigned char* pa = a;
    const long f0 = Counting::frees;
    Buf b(std::move(a));
    CHECK(!a && a.bytes() == 0 && (unsigned char*)b == pa && b.bytes() == 32 && Counting::frees == f0);
    Buf c;
    CHECK(c.regrow(48));
    unsigned char* pc = c;
    c = std::move(b);   // (c's own block goes, b's arrives)
    CHECK(!b && b.bytes() == 0 && (unsigned char*)c == pa && c.bytes() == 32 && Counting::frees == f0 + 1 && Counting::last_freed == pc);
    Buf& cr = c;
    c = std::move(cr);  // (self-assignment keeps it)
    CHECK((unsigned char*)c == pa && c.bytes() == 32 && Counting::frees == f0 + 1);
    Buf d;
    CHECK(d.regrow(8));
    unsigned char* pd = d;
    c.swap(d);
    CHECK((unsigned char*)c == pd && c.bytes() == 8 && (unsigned char*)d == pa && d.bytes() == 32 && Counting::frees == f0 + 1);
    CHECK(Counting::live == 2 && Counting::live_bytes == 40);
  }
  CHECK(Counting::live == 0 && Counting::live_bytes == 0);

  {   // a vector of structs that hold buffers: growth by emplace_back moves them, clear() frees them
    std::vector<Holder> v;
    std::vector<unsigned char*> first;
    for (int i = 0; i < 37; ++i) {
      Holder& h = v.emplace_back();
      h.id = i;
      CHECK(h.a.regrow(10 + i) && h.b.replace(5));
      h.a[0] = (unsigned char)i;
      first.push_back(h.a);
    }
    CHECK(Counting::live == 74 && Counting::live_bytes == 37 * 15 + 36 * 37 / 2);
    bool kept = true;
    for (int i = 0; i < 37; ++i) kept = kept && v[i].id == i && (unsigned char*)v[i].a == first[i] && v[i].a[0] == i && v[i].a.bytes() == (size_t)(10 + i);
    CHECK(kept);
    v[3] = Holder{};   // (how the host layer empties a tile set)
    CHECK(Counting::live == 72);
    v.clear();
    CHECK(Counting::live == 0 && Counting::live_bytes == 0);
  }

  CHECK(Counting::live == 0 && Counting::live_bytes == 0);
  if (g_failed) { std::printf("%d devmem checks FAILED\n", g_failed); return 1; }
  std::printf("all devmem checks passed\n");
  return 0;
}
