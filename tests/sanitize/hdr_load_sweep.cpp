// hdr_load_sweep.cpp — rts_hdr_load and rts_hdr_cache (csrc/host/rt_scene.cpp) under AddressSanitizer
// and UBSan, stand-alone (`make -C tests/sanitize`: g++ -fsanitize=address,undefined, no GPU, no Python).
//
// Writes Radiance .hdr files into a temporary directory and loads each: every scanline encoding the
// decoder reads (new-style RLE, flat, old-style 1,1,1,n repeat markers, the 2,2,x>=128 and 2,x
// starts) at widths on both sides of the new-style limits, every truncation of a few small files,
// broken headers, old-style runs longer than their scanline (the overrun the reference's
// oldDecrunch writes past its buffer with: RTS_ERR_FORMAT here), and a few thousand seeded byte
// mutations of small valid files, whose decoded images also go through rts_hdr_cache.  The values
// are tests/test_env_cases.py's business as well; here every load runs with the heap checked, and
// a returned image that nobody frees is a leak report at exit.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "rt_scene.h"

#define REQUIRE(x)                                                        \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #x);   \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

typedef std::vector<unsigned char> Bytes;
struct Px { unsigned char v[4]; };
typedef std::vector<Px> Image;  // h rows of w pixels

static std::string g_dir;
static long g_loads = 0, g_ok = 0, g_format = 0;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void put(Bytes& b, const char* s) { b.insert(b.end(), s, s + strlen(s)); }
static Bytes header(int w, int h, int variant) {
  Bytes b;
  put(b, "#?RADIANCE\n");
  if (variant == 1) put(b, "FORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n");
  if (variant == 2) put(b, "# a comment\nFORMAT=32-bit_rle_rgbe\n");
  char reso[64];
  snprintf(reso, sizeof reso, "\n-Y %d +X %d\n", h, w);
  put(b, reso);
  return b;
}

// Load one file.  rc must be RTS_OK or RTS_ERR_FORMAT; an error returns no image.  want (may be
// null): the expected floats of an RTS_OK load.
static int load(const Bytes& file, int want_rc, const std::vector<float>* want, bool cache) {
  const std::string path = g_dir + "/t.hdr";
  FILE* fp = fopen(path.c_str(), "wb");
  REQUIRE(fp);
  REQUIRE(file.empty() || fwrite(file.data(), 1, file.size(), fp) == file.size());
  fclose(fp);
  int32_t w = -7, h = -7;
  float* rgb = (float*)(uintptr_t)1;
  const int rc = rts_hdr_load(path.c_str(), &w, &h, &rgb);
  g_loads++;
  REQUIRE(rc == RTS_OK || rc == RTS_ERR_FORMAT);
  if (want_rc <= 0) REQUIRE(rc == want_rc);
  if (rc != RTS_OK) {
    REQUIRE(rgb == nullptr);
    g_format++;
    return rc;
  }
  g_ok++;
  REQUIRE(rgb && w > 0 && h > 0);
  const size_t n = (size_t)w * h * 3;
  if (want) {
    REQUIRE(want->size() == n);
    REQUIRE(memcmp(want->data(), rgb, n * sizeof(float)) == 0);
  }
  if (cache) {
    std::vector<float> out(n);
    REQUIRE(rts_hdr_cache(rgb, w, h, out.data()) == RTS_OK);
    for (size_t i = 0; i < n; i += 3)  // x and y are texel coordinates over the size, whatever the pdf
      REQUIRE(out[i] >= 0.0f && out[i] < 1.0f && out[i + 1] >= 0.0f && out[i + 1] <= 1.0f);
  }
  rts_free(rgb);
  return rc;
}

static std::vector<float> decode(const Image& im) {
  std::vector<float> out;
  for (const Px& p : im)
    for (int c = 0; c < 3; c++) out.push_back((float)ldexp((double)p.v[c], (int)p.v[3] - 136));
  return out;
}

static bool same(const Px& a, const Px& b) { return memcmp(a.v, b.v, 4) == 0; }

// Random pixels with the corner exponents and mantissas, stretches of one pixel (the first row one
// pixel throughout), and nothing a flat / old-style scanline cannot carry literally.
static Image pixels(int w, int h, int start /* 0 free, 1: 2,2,x>=128, 2: 2,x */, bool zero_start) {
  static const unsigned char es[6] = {0, 1, 127, 128, 129, 255};
  Image im((size_t)w * h);
  for (Px& p : im) {
    for (int c = 0; c < 4; c++) p.v[c] = (unsigned char)rnd();
    if (rnd() & 1) p.v[3] = es[rnd() % 6];
    for (int c = 0; c < 3; c++) {
      const uint32_t r = rnd() % 10;
      if (r == 0) p.v[c] = 0;
      if (r == 9) p.v[c] = 255;
    }
  }
  for (int y = 0; y < h; y++) {
    Px* row = &im[(size_t)y * w];
    const int a = rnd() % w, n = 2 + rnd() % 10;
    for (int x = a; x < w && x < a + n; x++) row[x] = row[a];
    if (y == 0 && h > 2) for (int x = 1; x < w; x++) row[x] = row[0];
    if (zero_start && y == h - 1) for (int x = 0; x < w && x < 3; x++) memset(row[x].v, 0, 4);
    for (int x = 0; x < w; x++)
      if (row[x].v[0] == 1 && row[x].v[1] == 1 && row[x].v[2] == 1) row[x].v[0] = 3;
    if (start == 1) { row[0].v[0] = 2; row[0].v[1] = 2; row[0].v[2] |= 128; }
    if (start == 2) { row[0].v[0] = 2; if (row[0].v[1] == 2) row[0].v[1] = 7; }
    if (start == 0 && row[0].v[0] == 2 && row[0].v[1] == 2) row[0].v[2] |= 128;
  }
  return im;
}

static void enc_flat(const Image& im, Bytes& b) {
  for (const Px& p : im) b.insert(b.end(), p.v, p.v + 4);
}
static void enc_old(const Image& im, int w, int h, Bytes& b) {
  for (int y = 0; y < h; y++) {
    const Px* row = &im[(size_t)y * w];
    Px prev = {{0, 0, 0, 0}};
    for (int j = 0; j < w;) {
      if (j > 0 || !same(row[0], prev)) {
        prev = row[j++];
        b.insert(b.end(), prev.v, prev.v + 4);
      }
      int k = j;
      while (k < w && same(row[k], prev)) k++;
      for (int n = k - j; n; n >>= 8) {
        const unsigned char m[4] = {1, 1, 1, (unsigned char)(n & 255)};
        b.insert(b.end(), m, m + 4);
      }
      j = k;
    }
  }
}
static void enc_rle(const Image& im, int w, int h, Bytes& b) {
  for (int y = 0; y < h; y++) {
    const Px* row = &im[(size_t)y * w];
    const unsigned char head[4] = {2, 2, (unsigned char)(w >> 8), (unsigned char)(w & 255)};
    b.insert(b.end(), head, head + 4);
    for (int c = 0; c < 4; c++) {
      Bytes lit;
      auto flush = [&] {
        if (lit.empty()) return;
        b.push_back((unsigned char)lit.size());
        b.insert(b.end(), lit.begin(), lit.end());
        lit.clear();
      };
      for (int j = 0; j < w;) {
        int k = j + 1;
        while (k < w && k - j < 127 && row[k].v[c] == row[j].v[c]) k++;
        if (k - j >= 3) {
          flush();
          b.push_back((unsigned char)(128 + k - j));
          b.push_back(row[j].v[c]);
          j = k;
        } else {
          lit.push_back(row[j++].v[c]);
          if (lit.size() == 128) flush();
        }
      }
      flush();
    }
  }
}

enum Mode { RLE, FLAT, OLD, FLAT_22X, FLAT_2X, N_MODES };
static Bytes make_file(int w, int h, int mode, int variant, Image* im_out) {
  Image im = pixels(w, h, mode == FLAT_22X ? 1 : mode == FLAT_2X ? 2 : 0, mode == OLD && h > 1);
  Bytes b = header(w, h, variant);
  if (mode == RLE) enc_rle(im, w, h, b);
  else if (mode == OLD) enc_old(im, w, h, b);
  else enc_flat(im, b);
  if (im_out) *im_out = im;
  return b;
}

static Bytes old_file(int w, int h, std::initializer_list<Px> px) {
  Bytes b = header(w, h, 1);
  for (const Px& p : px) b.insert(b.end(), p.v, p.v + 4);
  return b;
}
static Px M(int n) { return Px{{1, 1, 1, (unsigned char)n}}; }

int main() {
  char tmpl[] = "/tmp/hdr_load_sweep.XXXXXX";
  REQUIRE(mkdtemp(tmpl));
  g_dir = tmpl;
  static const int widths[] = {1, 7, 8, 9, 100, 300, 32767, 32768};

  // first the known hole: old-style runs past the end of their scanline (the reference copies them
  // past its buffer), and the same shapes where they just fit
  const Px P = {{9, 8, 7, 128}}, Q = {{30, 20, 10, 129}}, T = {{2, 5, 5, 128}};
  load(old_file(4, 1, {P, M(255)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 1, {P, M(4)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 1, {M(5)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 2, {P, M(3), Q, Q, M(3)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(300, 1, {P, M(40), M(2)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(100, 1, {P, M(1), M(1)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(300, 1, {P, M(0), M(0), M(1)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 1, {P, M(0), M(0), M(0), M(0), M(0), M(0), M(1)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 1, {P, M(0), M(0), M(0), M(255)}), RTS_ERR_FORMAT, nullptr, false);  // 255 << 24
  load(old_file(9, 1, {T, M(9)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(40000, 1, {P, M(255), M(255)}), RTS_ERR_FORMAT, nullptr, false);
  load(old_file(4, 1, {P, M(3)}), RTS_OK, nullptr, true);
  load(old_file(4, 1, {M(4)}), RTS_OK, nullptr, true);
  load(old_file(300, 1, {P, M(43), M(1)}), RTS_OK, nullptr, true);
  load(old_file(4, 1, {P, M(0), M(0), M(0), M(0), M(0), M(0), Q, M(2)}), RTS_OK, nullptr, true);
  load(old_file(9, 1, {T, M(8)}), RTS_OK, nullptr, true);
  load(old_file(40000, 1, {P, M(63), M(156)}), RTS_OK, nullptr, false);

  // well-formed files of every encoding
  for (int w : widths)
    for (int mode = 0; mode < N_MODES; mode++) {
      if (mode == RLE && (w < 8 || w > 0x7fff)) continue;
      for (int h = 1; h <= (w > 300 ? 2 : 5); h++) {
        Image im;
        const Bytes f = make_file(w, h, mode, (w + h + mode) % 3, &im);
        const std::vector<float> want = decode(im);
        load(f, RTS_OK, &want, w <= 300);
      }
    }

  // every truncation of small files: RTS_OK once the resolution line is whole, RTS_ERR_FORMAT before
  for (int w : {5, 9})
    for (int mode = 0; mode < N_MODES; mode++) {
      if (mode == RLE && w < 8) continue;
      const Bytes f = make_file(w, 3, mode, 1, nullptr);
      const size_t head = header(w, 3, 1).size();
      for (size_t cut = 0; cut < f.size(); cut++)
        load(Bytes(f.begin(), f.begin() + cut), cut < head ? RTS_ERR_FORMAT : RTS_OK, nullptr, true);
    }

  // broken headers
  for (const char* h : {"#?RADIANCX\nFORMAT=32-bit_rle_rgbe\n\n-Y 1 +X 1\n\1\2\3\200", "#?RADIAN",
                        "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n-Y 1 +X 1\n\1\2\3\200", "#?RADIANCE\nFORMAT=x\n\n-Y 1 +X 1",
                        "#?RADIANCE\nFORMAT=x\n\n+X 1 -Y 1\n\1\2\3\200", "#?RADIANCE\nFORMAT=x\n\n-Y 1\n\1\2\3\200",
                        "#?RADIANCE\nFORMAT=x\n\n-Y 1 +X 0\n\1\2\3\200", "#?RADIANCE\nFORMAT=x\n\n-Y 0 +X 1\n\1\2\3\200",
                        "#?RADIANCE\nFORMAT=x\n\n-Y 1 +X -4\n\1\2\3\200", "#?RADIANCE\nFORMAT=x\n\n-Y -1 +X 1\n\1\2\3\200"}) {
    Bytes b;
    put(b, h);
    load(b, RTS_ERR_FORMAT, nullptr, false);
  }

  // seeded byte mutations of small valid files.  The resolution line only swaps digits for digits
  // (the image stays small); everywhere else 1 to 3 bytes take random or format-significant values.
  static const unsigned char hot[] = {0, 1, 2, 127, 128, 129, 255, '\n'};
  long mutated = 0;
  for (int round = 0; round < 4000; round++) {
    static const int small[] = {1, 4, 7, 8, 9, 12, 40};
    const int w = small[rnd() % 7], h = 1 + rnd() % 4;
    int mode = rnd() % N_MODES;
    if (mode == RLE && w < 8) mode = OLD;
    const int variant = rnd() % 3;
    Bytes f = make_file(w, h, mode, variant, nullptr);
    const size_t head = header(w, h, variant).size();
    size_t reso = head - 2;
    while (f[reso - 1] != '\n') reso--;  // the resolution line is f[reso .. head)
    for (int k = 1 + rnd() % 3; k > 0; k--) {
      const size_t i = rnd() % f.size();
      if (i >= reso && i < head) {
        if (f[i] >= '0' && f[i] <= '9') f[i] = (unsigned char)('0' + rnd() % 10);
        continue;
      }
      f[i] = rnd() & 1 ? hot[rnd() % sizeof hot] : (unsigned char)rnd();
      if (rnd() % 8 == 0 && i >= head) {  // or the shape of a repeat marker
        const unsigned char m[4] = {1, 1, 1, (unsigned char)rnd()};
        for (size_t j = 0; j < 4 && i + j < f.size(); j++) f[i + j] = m[j];
      }
    }
    load(f, 1, nullptr, true);
    mutated++;
  }

  unlink((g_dir + "/t.hdr").c_str());
  rmdir(g_dir.c_str());
  printf("hdr_load_sweep: %ld loads (%ld mutations): %ld decoded, %ld refused as malformed\n", g_loads, mutated, g_ok,
         g_format);
  return 0;
}
