// guess_override_driver.cpp - lk_tracker_override_guesses and the frame-0 search hook of lk_sequence_frame /
// lk_sequence_run, on the host only: csrc/lk_tracker.cpp linked with the CPU mock of the engine (lk_engine_mock.cpp).
// The search is a stand-in that moves every guess by a fixed amount (the real one is lk_search_guesses, on the device).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lk_tracker.h"

extern "C" int lk_tracker_internal_set_search(lk_tracker *t, const lk_guess_search *cfg,
                                              int (*search)(lk_engine *, const lk_guess_search *, float *));

#define CHECK(c)                                                                                    \
  do {                                                                                              \
    if (!(c)) {                                                                                     \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c);                    \
      std::exit(1);                                                                                 \
    }                                                                                               \
  } while (0)

static int g_calls = 0;
static int fake_search(lk_engine *e, const lk_guess_search *cfg, float *guesses) {
  CHECK(e && cfg && guesses && cfg->radius == 7 && cfg->def_slot == -1);
  const int S = lk_sector_count(e);
  for (int s = 0; s < S; ++s) {
    guesses[6 * s] += 5.f;
    guesses[6 * s + 1] -= 3.f;
  }
  ++g_calls;
  return 0;
}

struct Frames {
  std::vector<std::vector<uint8_t>> px;
};
static const uint8_t *provide(void *user, int index, int *rows, int *cols, int *step, const char **name) {
  Frames *f = (Frames *)user;
  *rows = *cols = *step = 64;
  *name = nullptr;
  return f->px[(size_t)index].data();
}

int main() {
  lk_tracker_config cfg{};
  cfg.fitting_model = LK_FM_UVUXUYVXVY, cfg.domain_type = LK_DOMAIN_RECT, cfg.deformation = LK_DEF_EULERIAN;
  cfg.reference_image = LK_REF_FIRST, cfg.error_mode = LK_ERRMODE_CONTINUE;
  cfg.global_guess[0] = 1.5f, cfg.global_guess[1] = -0.5f, cfg.global_guess[2] = 0.01f;
  // the host-only override
  {
    lk_tracker *t = nullptr;
    CHECK(lk_tracker_create(&cfg, &t) == 0);
    CHECK(lk_tracker_set_rect_domain(t, 8.f, 8.f, 55.f, 55.f, 31.5f, 31.5f, 3, 2) == 0);
    const int S = lk_tracker_sector_count(t);
    std::vector<float> g(6 * (size_t)S, 0.f), mine(6 * (size_t)S, 0.f);
    for (int k = 0; k < 6 * S; ++k)
      mine[(size_t)k] = 0.25f * (float)k;
    CHECK(lk_tracker_override_guesses(t, mine.data()) == LK_ERROR_BAD_DOMAIN); // before begin_frame(0)
    std::vector<lk_sector_command> cmds((size_t)S);
    CHECK(lk_tracker_begin_frame(t, 0, cmds.data(), g.data()) == 0);
    CHECK(lk_tracker_override_guesses(t, nullptr) == LK_ERROR_BAD_DOMAIN);
    CHECK(lk_tracker_override_guesses(t, mine.data()) == 0);
    std::vector<lk_frame_result> res((size_t)S);
    CHECK(lk_tracker_get_results(t, res.data()) == 0);
    for (int s = 0; s < S; ++s)
      for (int p = 0; p < 6; ++p) {
        CHECK(res[(size_t)s].initial_guess[p] == mine[6 * (size_t)s + (size_t)p]);
        CHECK(res[(size_t)s].previous_resulting_parameters[p] == mine[6 * (size_t)s + (size_t)p]);
      }
    std::vector<lk_result> rec((size_t)S);
    std::memset(rec.data(), 0, rec.size() * sizeof(lk_result));
    int first = 0, stop = 0;
    CHECK(lk_tracker_end_frame(t, 0, "a", "b", rec.data(), &first, &stop) == 0);
    CHECK(lk_tracker_begin_frame(t, 1, cmds.data(), g.data()) == 0);
    CHECK(lk_tracker_override_guesses(t, mine.data()) == LK_ERROR_BAD_DOMAIN); // frame 1
    lk_tracker_destroy(t);
  }
  // the frame-0 hook: the synchronous path and the overlapped windows see the same searched guesses
  Frames f;
  unsigned seed = 9u;
  for (int i = 0; i < 5; ++i) {
    std::vector<uint8_t> p(64 * 64);
    for (auto &v : p)
      v = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
    f.px.push_back(p);
  }
  std::vector<lk_frame_result> first_res[2];
  for (int sync = 0; sync < 2; ++sync) {
    if (sync)
      setenv("LK_SEQ_SYNC", "1", 1);
    else
      unsetenv("LK_SEQ_SYNC");
    lk_config ec{LK_IM_BICUBIC, LK_FM_UVUXUYVXVY, 0.001f, 50, 0, 1, 2, 0};
    lk_engine *e = nullptr;
    CHECK(lk_create(&ec, &e) == 0);
    lk_tracker *t = nullptr;
    CHECK(lk_tracker_create(&cfg, &t) == 0);
    CHECK(lk_tracker_set_rect_domain(t, 8.f, 8.f, 55.f, 55.f, 31.5f, 31.5f, 3, 2) == 0);
    lk_guess_search gs{1, 7, 0, 0.f, 3};
    CHECK(lk_tracker_internal_set_search(t, &gs, &fake_search) == 0);
    const int calls = g_calls;
    int pairs = 0;
    CHECK(lk_sequence_run(e, t, 2, provide, &f, &pairs) == 0 && pairs == 1);
    CHECK(g_calls == calls + 1);
    const int S = lk_tracker_sector_count(t);
    first_res[sync].resize((size_t)S);
    CHECK(lk_tracker_get_results(t, first_res[sync].data()) == 0);
    lk_tracker_destroy(t);
    lk_destroy(e);
  }
  unsetenv("LK_SEQ_SYNC");
  CHECK(first_res[0].size() == first_res[1].size() && !first_res[0].empty());
  for (size_t s = 0; s < first_res[0].size(); ++s) {
    CHECK(std::memcmp(first_res[0][s].initial_guess, first_res[1][s].initial_guess, sizeof(float) * 6) == 0);
    CHECK(std::memcmp(first_res[0][s].previous_resulting_parameters, first_res[0][s].initial_guess, sizeof(float) * 6) == 0);
  }
  std::printf("guess_override_driver ok\n");
  return 0;
}
