// A C++ caller of Language / Script / TokenLanguageFilter / TdtDecoderV3 (include/fluidaudio.hpp), built with -Wall -Wextra -Werror by
// tests/test_tdt_lang_cpu.py.  No device: the class bytes are host work, and the decoding entry is only asked for its argument contract.
#include <cstdio>
#include <string>
#include <vector>

#include "fluidaudio.hpp"

using namespace fluidaudio;

int main() {
    const std::string marker = "\xE2\x96\x81";
    std::printf("MATCH %d %d %d %d %d %d\n", TokenLanguageFilter::matches("hello", Script::latin), TokenLanguageFilter::matches("hello \xD0\xBC\xD0\xB8\xD1\x80", Script::latin),
                TokenLanguageFilter::matches(marker + "\xD0\xBF\xD1\x80\xD0\xB8", Script::cyrillic), TokenLanguageFilter::matches(marker, Script::greek),
                TokenLanguageFilter::matches("cze\xC5\x9B\xC4\x87", Script::cyrillic), TokenLanguageFilter::matches("\xCE\xBB\xCF\x8C\xCE\xB3\xCE\xBF\xCF\x82", Script::greek));
    std::printf("LANG %s %d %s %d %s %d %s %d\n", rawValue(Language::polish), static_cast<int>(script(Language::polish)), rawValue(Language::russian),
                static_cast<int>(script(Language::russian)), rawValue(Language::serbian), static_cast<int>(script(Language::serbian)), rawValue(Language::greek),
                static_cast<int>(script(Language::greek)));
    std::printf("BLOCK %d %d %d\n", TdtDecoderV3::englishBlocklistApplies(Language::french), TdtDecoderV3::englishBlocklistApplies(Language::german),
                TdtDecoderV3::englishBlocklistApplies(std::nullopt));
    const std::vector<uint8_t> classes = TokenLanguageFilter::tokenClasses({std::string(" the"), std::nullopt, std::string("\xD0\xB8")}, {0});
    std::printf("CLASSES %d %d %d\n", classes[0], classes[1], classes[2]);
    int thrown = 0;
    try { TokenLanguageFilter::tokenClasses({std::string("\xC0\x80")}); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    try { TokenLanguageFilter::tokenClasses({std::string("a")}, {1}); } catch (const Error &e) { thrown += e.status == FA_INVALID_ARGUMENT; }
    std::printf("THROWN %d\n", thrown);
    // the entries without a context: a status, nothing thrown across the ABI
    fa_tdt_config cfg;
    fa_tdt_default_config(&cfg);
    std::printf("ST %d %d\n", static_cast<int>(fa_tdt_greedy_logits_lang_dev(nullptr, &cfg, nullptr, 0, 1, 1, 1, 1, 6, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                                                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 64, nullptr,
                                                                              nullptr)),
                static_cast<int>(fa_tdt_topk_rows_dev(nullptr, nullptr, 0, 1, 1, 1, 1, nullptr, nullptr, nullptr)));
    return 0;
}
