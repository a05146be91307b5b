// call_order_main.cpp -- TEST INFRASTRUCTURE ONLY (see prim_sim.hpp).
// A stand-alone program for an AddressSanitizer build of the serial stand-in (make -C tests/hostsim call_order_asan): it
// replays, through the C ABI, every sequence of one to three stage calls in which the call-order contract of
// include/grlbwt_hip.h refuses a call or makes it a no-op, and checks every return code against a model of that contract
// written here from the table alone.  After each sequence grlbwt_result_size must succeed exactly in DONE, and a final
// grlbwt_build must give the image of a plain build.  Exit status 0: every sequence behaved; a refused call that reads
// released memory ends the program in the sanitizer's report instead.
#include "engine_sim.cpp"

#include <cstdio>
#include <cstdlib>

namespace {

enum Call { PARSE_ROUND, PARSE_PHASE, INDUCE_FIRST, INDUCE_LEVEL, INDUCE_PHASE, BUILD, N_CALLS };
const char *const kCallName[N_CALLS] = {"parse_round", "parse_phase", "induce_first", "induce_level", "induce_phase", "build"};
enum State { LOADED, PARTLY_PARSED, PARSED, INDUCING, DONE };
const char *const kStateName[] = {"LOADED", "PARTLY PARSED", "PARSED", "INDUCING", "DONE"};
enum Kind { ADVANCE, NOOP, REFUSED };

// the table of include/grlbwt_hip.h; `rounds` = the parsing rounds of the text
struct Model {
    int rounds;
    State st = LOADED;
    int parsed = 0, level = -1;
    Kind step(Call c) {
        const bool parsing = st == LOADED || st == PARTLY_PARSED;
        switch (c) {
            case PARSE_ROUND:
                if (!parsing) return NOOP;
                st = ++parsed == rounds ? PARSED : PARTLY_PARSED;
                return ADVANCE;
            case PARSE_PHASE:
                if (!parsing) return NOOP;
                parsed = rounds; st = PARSED;
                return ADVANCE;
            case INDUCE_FIRST:
                if (st != PARSED) return REFUSED;
                level = rounds; st = INDUCING;
                return ADVANCE;
            case INDUCE_LEVEL:
                if (st != INDUCING) return REFUSED;
                if (--level == 0) st = DONE;
                return ADVANCE;
            case INDUCE_PHASE:
                if (parsing) return REFUSED;
                if (st == DONE) return NOOP;
                st = DONE;
                return ADVANCE;
            default:
                if (st == DONE) return NOOP;
                st = DONE;
                return ADVANCE;
        }
    }
};

int call(grlbwt_ctx *ctx, Call c) {
    int done = 0, n = 0, level = 0;
    grlbwt_round_info ri;
    grlbwt_level_info li;
    switch (c) {
        case PARSE_ROUND: return grlbwt_parse_round(ctx, &ri, &done);
        case PARSE_PHASE: return grlbwt_parse_phase(ctx, &n);
        case INDUCE_FIRST: return grlbwt_induce_first(ctx);
        case INDUCE_LEVEL: return grlbwt_induce_level(ctx, &level, &li);
        case INDUCE_PHASE: return grlbwt_induce_phase(ctx);
        default: return grlbwt_build(ctx);
    }
}

// reads drawn from a short genome: a few hundred strings that share long pieces, so the parse takes several rounds
std::vector<uint8_t> reads_text() {
    uint64_t s = 20260011;
    auto next = [&] { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
    std::vector<uint8_t> genome(3000), text;
    for (auto &g : genome) g = "ACGT"[next() & 3];
    for (int i = 0; i < 400; i++) {
        const uint32_t at = next() % (uint32_t)(genome.size() - 80);
        text.insert(text.end(), genome.begin() + at, genome.begin() + at + 80);
        text.push_back('\n');
    }
    return text;
}

std::vector<uint8_t> image_of(grlbwt_ctx *ctx) {
    uint64_t nb = 0;
    if (grlbwt_result_size(ctx, &nb, nullptr) != GRLBWT_OK) return {};
    std::vector<uint8_t> out(nb);
    if (grlbwt_result_download(ctx, out.data(), nb) != GRLBWT_OK) return {};
    return out;
}

}   // namespace

int main() {
    const std::vector<uint8_t> text = reads_text();
    grlbwt_ctx *ctx = nullptr;
    if (grlbwt_ctx_create(0, 0, &ctx) != GRLBWT_OK) { fprintf(stderr, "no context\n"); return 2; }
    // the text's rounds and its image, by the canonical order
    int rounds = 0, done = 0;
    if (grlbwt_text_upload(ctx, text.data(), text.size(), 1) != GRLBWT_OK) return 2;
    while (!done) { if (grlbwt_parse_round(ctx, nullptr, &done) != GRLBWT_OK) return 2; rounds++; }
    if (grlbwt_induce_phase(ctx) != GRLBWT_OK) return 2;
    const std::vector<uint8_t> want = image_of(ctx);
    if (rounds < 3 || want.empty()) { fprintf(stderr, "the text parses in %d rounds: too few to reach every state\n", rounds); return 2; }
    printf("text: %zu cells, %d parsing rounds, image %zu bytes\n", text.size(), rounds, want.size());

    int replayed = 0, bad = 0;
    for (int len = 1; len <= 3; len++) {
        int total = 1;
        for (int i = 0; i < len; i++) total *= N_CALLS;
        for (int code = 0; code < total; code++) {
            Call seq[3];
            for (int i = 0, c = code; i < len; i++, c /= N_CALLS) seq[i] = (Call)(c % N_CALLS);
            Model probe{rounds};
            bool wanted = false;
            for (int i = 0; i < len; i++) wanted = probe.step(seq[i]) != ADVANCE || wanted;
            if (!wanted) continue;
            replayed++;
            std::string name;
            for (int i = 0; i < len; i++) name += std::string(i ? ", " : "") + kCallName[seq[i]];
            fflush(stdout);
            fprintf(stderr, "replaying: %s\n", name.c_str());      // (unbuffered: the last line names the sequence a fault ends)
            if (grlbwt_text_upload(ctx, text.data(), text.size(), 1) != GRLBWT_OK) return 2;
            Model m{rounds};
            bool ok = true;
            for (int i = 0; i < len && ok; i++) {
                const Kind k = m.step(seq[i]);
                const int rc = call(ctx, seq[i]);
                if ((k == REFUSED) != (rc == GRLBWT_EINVAL) || (k != REFUSED && rc != GRLBWT_OK)) {
                    printf("FAIL %s: call %d returned %d, the model says %s\n", name.c_str(), i, rc, k == REFUSED ? "EINVAL" : "OK");
                    ok = false;
                }
                if (k == REFUSED && rc == GRLBWT_EINVAL && !*grlbwt_last_error(ctx)) { printf("FAIL %s: call %d refused without a message\n", name.c_str(), i); ok = false; }
            }
            uint64_t nb = 0;
            if (ok && (grlbwt_result_size(ctx, &nb, nullptr) == GRLBWT_OK) != (m.st == DONE)) {
                printf("FAIL %s: grlbwt_result_size does not agree with the model's state %s\n", name.c_str(), kStateName[m.st]);
                ok = false;
            }
            if (ok && (grlbwt_build(ctx) != GRLBWT_OK || image_of(ctx) != want)) { printf("FAIL %s: the build afterwards does not give the image\n", name.c_str()); ok = false; }
            if (!ok) bad++;
        }
    }
    grlbwt_ctx_destroy(ctx);
    printf("%d sequences with a refused or no-op call replayed, %d failed\n", replayed, bad);
    return bad ? 1 : 0;
}
