// The plan and the EOS machine of the PocketTTS session (fluidaudio_amd/csrc/pockettts_core.h, the same source the GPU compiles) against
// the reference's loops written out naively: the machine on every pattern of eosLogit above / at / below the threshold over up to 10
// steps and three framesAfterEos; the windows for every block length up to 600 rows with and without a voice block; the clip plan.
// Prints "ok <cases>" or the first difference.
#include <cstdio>
#include <vector>

#include "../../fluidaudio_amd/csrc/pockettts_core.h"

using namespace fa::pockettts;

int main() {
    int cases = 0;
    const float levels[3] = {-9.0f, -4.0f, 1.0f};   // below, exactly the threshold (not EOS), above
    for (int after = 0; after <= 3; after += (after ? 2 : 1))
        for (int n = 0; n <= 10; ++n)
            for (int code = 0, codes = 1 << n; code < codes; ++code, ++cases) {
                std::vector<float> logit(n);
                for (int t = 0; t < n; ++t) logit[t] = levels[(code >> t & 1) ? 2 : (t % 2)];
                // PocketTtsSynthesizer.swift:535-568
                std::vector<int> emitted;
                int eos = -1, reason = kEndMaxLen;
                for (int step = 0; step < n; ++step) {
                    if (logit[step] > -4.0f && eos < 0) eos = step;
                    if (eos >= 0 && step >= eos + after + 2) { reason = kEndEos; break; }
                    emitted.push_back(step);
                }
                StreamState m = begin_state(n, after);
                std::vector<int> got;
                for (int t = 0; t < n + 2; ++t) {   // the calls past the end change nothing
                    const int step = m.step;
                    const bool emit = advance(m, t < n ? logit[t] : 1.0f);
                    if (emit) got.push_back(step);
                    if (m.emit != (emit ? 1 : 0)) { printf("emit flag: after %d n %d code %d t %d\n", after, n, code, t); return 1; }
                }
                if (got != emitted || m.reason != reason || m.eos_step != eos || m.frames != static_cast<int>(emitted.size())) {
                    printf("machine: after %d n %d code %d: %zu frames for %zu, reason %d for %d, eos %d for %d\n", after, n, code, got.size(), emitted.size(), m.reason, reason, m.eos_step, eos);
                    return 1;
                }
            }
    for (int prompt = 0; prompt <= 125; prompt += 125)
        for (int snapshot = 0; snapshot < 2; ++snapshot)
            for (int tokens = 0; tokens <= 600; ++tokens, ++cases) {
                std::vector<Window> w(8);
                int32_t count = 0;
                const VoiceFacts v{1, snapshot, prompt};
                if (plan_stream(3, 1, v, true, tokens, 11, w.data(), 8, &count) != kOk) { printf("plan refused: prompt %d tokens %d\n", prompt, tokens); return 1; }
                // KVCache :206-239 per block, the voice block first (:482-500)
                const int rows[2] = {!snapshot && prompt > 0 ? 1 + prompt : 0, tokens};
                int at = 0, before = 0;
                for (int block = 0; block < 2; ++block)
                    for (int processed = 0; processed < rows[block];) {
                        const int n = rows[block] - processed < 256 ? rows[block] - processed : 256;
                        const Window &x = w[at++];
                        if (at > count || x.stream != 3 || x.voice != 1 || x.ids_at != 11 || x.block != block || x.first != processed || x.n != n || x.before != before) {
                            printf("window %d: prompt %d snapshot %d tokens %d\n", at - 1, prompt, snapshot, tokens);
                            return 1;
                        }
                        processed += n;
                        before += n;
                    }
                if (at != count) { printf("window count %d for %d\n", count, at); return 1; }
            }
    {   // the statuses: no voice, no bos_before_voice for a cloned voice, a full arena
        std::vector<Window> w(2);
        int32_t count = 0;
        if (plan_stream(0, 0, VoiceFacts{0, 0, 0}, true, 5, 0, w.data(), 2, &count) != kNoVoice || plan_stream(0, 0, VoiceFacts{1, 0, 9}, false, 5, 0, w.data(), 2, &count) != kNoBosBeforeVoice ||
            plan_stream(0, 0, VoiceFacts{1, 0, 9}, true, 257, 0, w.data(), 2, &count) != kTooManyWindows || count != 0 || plan_stream(0, 0, VoiceFacts{1, 1, 9}, false, 257, 0, w.data(), 2, &count) != kOk) {
            printf("plan statuses\n");
            return 1;
        }
        ++cases;
    }
    for (int64_t samples = 0; samples <= 300000; samples += 37, ++cases) {   // VoiceCloner :137-148, :296-299
        const int64_t real = samples < 240000 ? samples : 240000;
        int64_t want = (real + 1919) / 1920;
        want = want < 100 ? want : 100;
        if (clip_status(samples) != (samples >= 24000 ? kOk : kClipTooShort) || usable_frames(samples, 100) != want || usable_frames(samples, 200) != (real + 1919) / 1920) {
            printf("clip plan: %lld samples\n", static_cast<long long>(samples));
            return 1;
        }
    }
    printf("ok %d\n", cases);
    return 0;
}
