// Host-side check of the round kernel's lane table (csrc/sgn_internal.h: ktab_src, ktab_reg,
// ktab_lane, ktab_pack, ktab_read): a DevSim with a distinct value in every byte is packed into
// the table's (register, lane) image and every field of the accessor's list is read back through
// the table's index arithmetic and compared with the struct member.
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "sgn_internal.h"

using sgn::DevSim;

struct Wide {  // a 24-byte field image: placed by hand across the 256-byte register boundaries
  uint64_t a;
  uint32_t b, c;
  uint64_t d;
};

int main() {
  long n = 0, bad = 0;
  // a distinct value per byte (the struct is under 1024 bytes: two passes of a 16-bit pattern)
  static_assert(sizeof(DevSim) <= 1024 && sizeof(DevSim) % 4 == 0, "");
  DevSim s;
  unsigned char* raw = (unsigned char*)&s;
  for (size_t i = 0; i < sizeof(DevSim); i++) raw[i] = (unsigned char)((i * 167u + (i >> 8) * 59u + 13u) & 0xFF);
  // (the pattern makes every aligned dword of the struct different from every other)
  for (size_t i = 0; i + 4 <= sizeof(DevSim); i += 4)
    for (size_t j = i + 4; j + 4 <= sizeof(DevSim); j += 4)
      if (!memcmp(raw + i, raw + j, 4)) {
        printf("pattern repeats at %zu and %zu\n", i, j);
        bad++;
      }
  sgn::KTabImage img;
  sgn::ktab_pack(s, &img);

  // the fill: every dword of the struct lands in its lane, and no lane reads past the struct
  for (uint32_t j = 0; j < sgn::KTAB_REGS; j++)
    for (uint32_t i = 0; i < 64; i++) {
      const uint32_t src = sgn::ktab_src(j, i);
      n++;
      if (src >= sgn::KTAB_DWORDS || (64 * j + i < sgn::KTAB_DWORDS && src != 64 * j + i)) {
        printf("fill: register %u lane %u reads dword %u\n", j, i, src);
        bad++;
      }
    }
  for (uint32_t d = 0; d < sgn::KTAB_DWORDS; d++) {
    uint32_t v;
    memcpy(&v, raw + 4 * d, 4);
    n++;
    if (sgn::ktab_reg(4 * d) >= sgn::KTAB_REGS || img.r[sgn::ktab_reg(4 * d)][sgn::ktab_lane(4 * d)] != v) {
      printf("dword %u is not at (register %u, lane %u)\n", d, sgn::ktab_reg(4 * d), sgn::ktab_lane(4 * d));
      bad++;
    }
  }

  // every field of the accessor's list, by its type and offsetof: u32, i32, u64, pointers, UDiv64
  int n64 = 0, nptr = 0, ndiv = 0, n32 = 0;
#define CHECK_FIELD(f)                                                                \
  {                                                                                   \
    using T = decltype(DevSim::f);                                                    \
    const T got = sgn::ktab_read<T>(img, (uint32_t)offsetof(DevSim, f));              \
    n++;                                                                              \
    if (memcmp(&got, &s.f, sizeof(T))) {                                              \
      printf("field %s (offset %zu, %zu bytes) differs\n", #f, offsetof(DevSim, f), sizeof(T)); \
      bad++;                                                                          \
    }                                                                                 \
    if (std::is_pointer<T>::value) nptr++;                                            \
    else if (std::is_same<T, sgn::UDiv64>::value) ndiv++;                             \
    else if (sizeof(T) == 8) n64++;                                                   \
    else if (sizeof(T) == 4) n32++;                                                   \
  }
  SGN_KTAB_FIELDS(CHECK_FIELD)
#undef CHECK_FIELD
  if (n64 < 10 || nptr < 40 || ndiv != 5 || n32 < 30) {
    printf("the field list is short: %d u64, %d pointers, %d UDiv64, %d dwords\n", n64, nptr, ndiv, n32);
    bad++;
  }
  // the array read element by element (SKE in engine.hip)
  for (uint32_t i = 0; i < 3; i++) {
    const uint64_t got = sgn::ktab_read<uint64_t>(img, (uint32_t)(offsetof(DevSim, file_bytes) + 8 * i));
    n++;
    if (got != s.file_bytes[i]) {
      printf("file_bytes[%u] differs\n", i);
      bad++;
    }
  }
  // a field across a register boundary: 24 bytes placed at every dword offset from 20 bytes
  // before a 256-byte boundary to the boundary itself (its dwords come from two registers)
  for (uint32_t b = 256; b < sizeof(DevSim); b += 256)
    for (uint32_t off = b - 20; off <= b && off + sizeof(Wide) <= sizeof(DevSim); off += 4) {
      Wide want;
      memcpy(&want, raw + off, sizeof(Wide));
      const Wide got = sgn::ktab_read<Wide>(img, off);
      n++;
      if (sgn::ktab_reg(off) == sgn::ktab_reg(off + sizeof(Wide) - 4) && off != b) {
        printf("offset %u does not straddle\n", off);
        bad++;
      }
      if (memcmp(&got, &want, sizeof(Wide))) {
        printf("straddling field at offset %u differs\n", off);
        bad++;
      }
    }
  printf("%ld checks, %ld bad\n", n, bad);
  return bad != 0;
}
