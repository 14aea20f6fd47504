// dcrt_render -- a C++ host of the MI355X wavefront path tracer in the shape of the reference's
// application: CScene + the CPathTracer plugin slot filled by CMI355XPathTracer
// (mi355x_path_tracer.h, the C ABI of include/dcrt.h alone) and the reference's frame loop
// (renderer_loop.h: LoadScene, DispatchRayTracing with its small-resolution first frame and
// frame-seed policies, SampleConvolution of each completed image), then "Save Image to File".
//
//   dcrt_render <scene.obj|scene.xml> <width> <height> <spp> <max_bounce> <out.bmp>
//               [--batch] [--point x y z r g b] [--seed-type sample-count|frame-index|fixed]
//               [--fixed-seed N] [--iterations N] [--pool N] [--film out.f32] [--samples out.f32]
//               [--edit N:KIND:ARGS]... [--output NAME [--iteration-threshold N]] [--denoise]
//               [--converge THRESHOLD[:FRACTION] [--check-points MIN:INTERVAL]] [--noise-map out.bmp]
//               [--adaptive THRESHOLD:FRACTION[:MARGIN]] [--sample-map out.bmp] [--env-importance]
//               [--roulette START[:MIN[:MAX]]] [--light-power] [--firefly [K:START:BASE:KAPPA]]
//
// --firefly keeps K cascade films beside the film and writes the BMP from the re-weighted image (dcrt.h "firefly
// re-weighting"; without the fields: dcrt_firefly_default_params, which come from a synthetic prototype and not from
// a render). With --denoise the re-weighted image is the denoiser's colour input (dcrt_tracer_denoise_firefly). --film still writes the film, which
// the feature never alters. The JSON line gains "firefly": the parameters and the share of the film's summed
// luminance that the resolve removed.
//
// --light-power picks the light of every light sample in proportion to the lights' power, and a lamp's triangle in
// proportion to its area, instead of uniformly (dcrt.h "light selection").
//
// --roulette turns Russian roulette on from bounce START (dcrt.h "Russian roulette"): a path survives a vertex with
// the probability clamp(max throughput component, MIN, MAX), defaults 0.05 and 1, and survivors are weighted up.
//
// --env-importance draws the light samples of an environment cube by its power instead of uniformly
// (dcrt.h "environment importance sampling"); a scene without a cube renders as without the flag.
//
// --adaptive runs like --converge (the same check points, --noise-map, "converged" and "noise"),
// but through dcrt_tracer_render_adaptive: after every check point only the 8 x 8 pixel blocks
// within MARGIN pixels (default: the filter's window rows) of a pixel that is still over
// THRESHOLD go on being traced (dcrt.h "adaptive sampling"). The JSON line gains "adaptive".
// --sample-map writes the film's weight over its maximum as a grey image, the per-pixel sampling
// density (code = (int)(v * 255 + 0.5)); it works with any mode.
//
// --converge renders until the half-film noise estimate (dcrt.h "film noise estimate") says that
// FRACTION (default 0.95) of the pixels have an error of at most THRESHOLD, checked at MIN, MIN +
// INTERVAL, ... images (default 16:16), and at most `spp` images (dcrt_tracer_render_converged;
// implies the --batch path). The JSON line's "images" is the count rendered, and it gains
// "converged" and "noise". --noise-map writes a grey image of min(e / THRESHOLD, 1) per pixel
// (code = (int)(v * 255 + 0.5); a NaN e is white).
//
// --denoise renders the denoiser's guide films (first-hit normal and albedo) with the seeds of the
// film's images, filters the film with the default parameters (dcrt_tracer_denoise) and writes the
// BMP from the denoised image; --film still writes the unfiltered film. Path tracing only.
//
// --output selects the tracer's "Output" view, in either mode: path_tracing (default), normal,
// tangent, albedo, negative_ndotv, backface or iteration_count (BVH node visits of the camera
// ray over --iteration-threshold, default 20, as a grey level; red above it). The film,
// post-processing and the BMP are as for a path-traced image.
//
// --edit (repeatable, frame loop only) edits the scene after N full-resolution images have
// completed since the start or the previous edit: material:INDEX:TYPE:R,G,B:ROUGHNESS,
// opacity:INDEX:VALUE, point:X,Y,Z:R,G,B (adds a point light), movepoint:INDEX:X,Y,Z,
// camera:X,Y,Z. The frame loop takes the edit as the reference's does (a preview frame, the
// film restarted, only the edited array sent); the run ends once `spp` images have completed
// after the last edit, and the JSON line gains "edits_applied" and "upload_stats".
//
// Frame-loop mode (default) runs frames until `spp` full-resolution images are in the film;
// --batch instead hands all images to dcrt_tracer_render_images (device-side image
// sequencing). --film writes the raw RGBA32F film (sum w*L, sum w), --samples the last image's
// sample textures (positions W*H*2 then values W*H*4 floats). The last stdout line is JSON.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dcrt.h"
#include "mi355x_path_tracer.h"
#include "renderer_loop.h"

namespace {

bool Check(int rc, const char* what)
{
    if (rc == DCRT_OK) return true;
    std::fprintf(stderr, "%s failed (%d): %s\n", what, rc, dcrt_last_error());
    return false;
}

bool WriteFloats(const char* path, const std::vector<float>& a, const std::vector<float>* b = nullptr)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    bool ok = std::fwrite(a.data(), sizeof(float), a.size(), f) == a.size();
    if (ok && b) ok = std::fwrite(b->data(), sizeof(float), b->size(), f) == b->size();
    return std::fclose(f) == 0 && ok;
}

int Usage(const char* exe)
{
    std::fprintf(stderr,
                 "usage: %s scene.{obj,xml} width height spp max_bounce out.bmp [--batch] [--point x y z r g b]\n"
                 "       [--seed-type sample-count|frame-index|fixed] [--fixed-seed N] [--iterations N] [--pool N]\n"
                 "       [--film out.f32] [--samples out.f32] [--edit N:KIND:ARGS]...\n"
                 "       [--output path_tracing|normal|tangent|albedo|negative_ndotv|backface|iteration_count]\n"
                 "       [--iteration-threshold N] [--denoise]\n"
                 "       [--converge THRESHOLD[:FRACTION] [--check-points MIN:INTERVAL]] [--noise-map out.bmp]\n"
                 "       [--adaptive THRESHOLD:FRACTION[:MARGIN]] [--sample-map out.bmp] [--env-importance]\n"
                 "       [--roulette START[:MIN[:MAX]]] [--light-power] [--firefly [K:START:BASE:KAPPA]]\n",
                 exe);
    return 2;
}

// --edit N:KIND:ARGS -- a scene edit the frame loop applies after N full-resolution images have
// completed since the start or the previous edit, as the reference's UI would between two frames
struct SEdit {
    uint32_t m_AfterImages = 0;
    std::string m_Kind;
    std::vector<std::string> m_Args;   // the ':'-separated fields after KIND
};

std::vector<std::string> Split(const std::string& s, char sep)
{
    std::vector<std::string> out;
    size_t start = 0;
    for (;;) {
        const size_t end = s.find(sep, start);
        out.push_back(s.substr(start, end == std::string::npos ? std::string::npos : end - start));
        if (end == std::string::npos) return out;
        start = end + 1;
    }
}

bool ParseFloats(const std::string& s, float* out, size_t count)
{
    const std::vector<std::string> parts = Split(s, ',');
    if (parts.size() != count) return false;
    for (size_t i = 0; i < count; ++i) {
        char* end = nullptr;
        out[i] = std::strtof(parts[i].c_str(), &end);
        if (end == parts[i].c_str() || *end) return false;
    }
    return true;
}

bool ParseEdit(const char* text, SEdit* edit)
{
    const std::vector<std::string> f = Split(text, ':');
    if (f.size() < 3) return false;
    char* end = nullptr;
    edit->m_AfterImages = (uint32_t)std::strtoul(f[0].c_str(), &end, 10);
    if (end == f[0].c_str() || *end) return false;
    edit->m_Kind = f[1];
    edit->m_Args.assign(f.begin() + 2, f.end());
    const size_t n = edit->m_Args.size();
    return (edit->m_Kind == "material" && n == 4) || (edit->m_Kind == "opacity" && n == 2) || (edit->m_Kind == "point" && n == 2) ||
           (edit->m_Kind == "movepoint" && n == 2) || (edit->m_Kind == "camera" && n == 1);
}

// The edit through the kept host API: the setters re-flatten their own arrays and leave the
// dirty bits CScene::AcquireEdits moves into the frame loop's flags.
bool ApplyEdit(dcrt_scene* scene, const SEdit& e)
{
    const std::vector<std::string>& a = e.m_Args;
    if (e.m_Kind == "material") {   // material:INDEX:TYPE:R,G,B:ROUGHNESS
        const uint32_t index = (uint32_t)std::atoi(a[0].c_str());
        float albedo[3];
        dcrt_material_setting m;
        if (!ParseFloats(a[2], albedo, 3) || !Check(dcrt_scene_get_material_setting(scene, index, &m), "GetMaterialSetting")) return false;
        return Check(dcrt_scene_set_material(scene, index, std::atoi(a[1].c_str()), albedo, (float)std::atof(a[3].c_str()), nullptr,
                                             nullptr, (int)m.multiscattering, (int)m.is_two_sided),
                     "SetMaterial");
    }
    if (e.m_Kind == "opacity") {    // opacity:INDEX:VALUE
        const uint32_t index = (uint32_t)std::atoi(a[0].c_str());
        dcrt_material_setting m;
        if (!Check(dcrt_scene_get_material_setting(scene, index, &m), "GetMaterialSetting")) return false;
        return Check(dcrt_scene_set_material_opacity(scene, index, (float)std::atof(a[1].c_str()), m.opacity_texture_index),
                     "SetMaterialOpacity");
    }
    if (e.m_Kind == "point") {      // point:X,Y,Z:R,G,B
        float position[3], color[3];
        const float euler[3] = {0, 0, 0};
        if (!ParseFloats(a[0], position, 3) || !ParseFloats(a[1], color, 3)) return false;
        return Check(dcrt_scene_add_punctual_light(scene, position, euler, color, 0), "AddPointLight");
    }
    if (e.m_Kind == "movepoint") {  // movepoint:INDEX:X,Y,Z
        const uint32_t index = (uint32_t)std::atoi(a[0].c_str());
        float old[3], euler[3], color[3], position[3];
        int directional = 0;
        if (!ParseFloats(a[1], position, 3) ||
            !Check(dcrt_scene_get_punctual_light(scene, index, old, euler, color, &directional), "GetPunctualLight"))
            return false;
        return Check(dcrt_scene_set_punctual_light(scene, index, position, euler, color, directional), "SetPunctualLight");
    }
    if (e.m_Kind == "camera") {     // camera:X,Y,Z
        float position[3];
        dcrt_scene_settings settings;
        if (!ParseFloats(a[0], position, 3) || !Check(dcrt_scene_get_settings(scene, &settings), "GetSettings")) return false;
        return Check(dcrt_scene_set_camera(scene, position, settings.camera_euler_angles), "SetCamera");
    }
    return false;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 7) return Usage(argv[0]);
    const char* scenePath = argv[1];
    const uint32_t width = (uint32_t)std::atoi(argv[2]), height = (uint32_t)std::atoi(argv[3]);
    const uint32_t spp = (uint32_t)std::atoi(argv[4]), maxBounce = (uint32_t)std::atoi(argv[5]);
    const char* outPath = argv[6];
    bool batch = false, pointLight = false, denoise = false;
    float lightPos[3] = {0, 0, 0}, lightColor[3] = {0, 0, 0};
    CRendererLoop::EFrameSeedType seedType = CRendererLoop::EFrameSeedType::SampleCount;
    uint32_t fixedSeed = 0, iterations = 16, pool = 0;
    const char* filmPath = nullptr;
    const char* samplesPath = nullptr;
    std::vector<SEdit> edits;
    uint32_t outputType = DCRT_OUTPUT_PATH_TRACING, iterationThreshold = 20;
    bool converge = false;
    dcrt_converge_params convergeParams = {0.0f, 0.95f, 16u, 0u, 16u};
    const char* noiseMapPath = nullptr;
    bool adaptive = false;
    bool firefly = false;
    dcrt_firefly_params fireflyParams;
    if (!Check(dcrt_firefly_default_params(&fireflyParams), "FireflyDefaultParams")) return 1;
    uint32_t adaptiveMargin = 0xFFFFFFFFu;   // (the filter's window rows)
    const char* sampleMapPath = nullptr;
    bool envImportance = false;
    bool lightPower = false;
    dcrt_roulette_params roulette;
    if (dcrt_roulette_default_params(&roulette) != DCRT_OK) return 1;
    for (int i = 7; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!std::strcmp(argv[i], "--batch")) {
            batch = true;
        } else if (!std::strcmp(argv[i], "--denoise")) {
            denoise = true;
        } else if (!std::strcmp(argv[i], "--env-importance")) {
            envImportance = true;
        } else if (!std::strcmp(argv[i], "--light-power")) {
            lightPower = true;
        } else if (!std::strcmp(argv[i], "--roulette") && more) {
            const std::vector<std::string> f = Split(argv[++i], ':');
            if (f.empty() || f.size() > 3 || f[0].empty() || f[0].find_first_not_of("0123456789") != std::string::npos ||
                (f.size() >= 2 && !ParseFloats(f[1], &roulette.min_survival, 1)) || (f.size() == 3 && !ParseFloats(f[2], &roulette.max_survival, 1)))
                return Usage(argv[0]);
            roulette.start_bounce = (uint32_t)std::atoi(f[0].c_str());
            roulette.enable = 1u;
        } else if (!std::strcmp(argv[i], "--point") && i + 6 < argc) {
            pointLight = true;
            for (int k = 0; k < 3; ++k) lightPos[k] = (float)std::atof(argv[i + 1 + k]);
            for (int k = 0; k < 3; ++k) lightColor[k] = (float)std::atof(argv[i + 4 + k]);
            i += 6;
        } else if (!std::strcmp(argv[i], "--seed-type") && more) {
            const std::string v = argv[++i];
            if (v == "sample-count") seedType = CRendererLoop::EFrameSeedType::SampleCount;
            else if (v == "frame-index") seedType = CRendererLoop::EFrameSeedType::FrameIndex;
            else if (v == "fixed") seedType = CRendererLoop::EFrameSeedType::Fixed;
            else return Usage(argv[0]);
        } else if (!std::strcmp(argv[i], "--fixed-seed") && more) {
            fixedSeed = (uint32_t)std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--iterations") && more) {
            iterations = (uint32_t)std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--pool") && more) {
            pool = (uint32_t)std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--film") && more) {
            filmPath = argv[++i];
        } else if (!std::strcmp(argv[i], "--samples") && more) {
            samplesPath = argv[++i];
        } else if (!std::strcmp(argv[i], "--output") && more) {
            static const char* const kOutputNames[] = {"path_tracing", "normal", "tangent", "albedo", "negative_ndotv", "backface",
                                                       "iteration_count"};   // DCRT_OUTPUT_* order
            const char* name = argv[++i];
            outputType = ~0u;
            for (uint32_t k = 0; k < 7; ++k)
                if (!std::strcmp(name, kOutputNames[k])) outputType = k;
            if (outputType == ~0u) return Usage(argv[0]);
        } else if (!std::strcmp(argv[i], "--iteration-threshold") && more) {
            iterationThreshold = (uint32_t)std::atoi(argv[++i]);
        } else if (!std::strcmp(argv[i], "--converge") && more) {
            const std::vector<std::string> f = Split(argv[++i], ':');
            if (f.size() > 2 || !ParseFloats(f[0], &convergeParams.threshold, 1) ||
                (f.size() == 2 && !ParseFloats(f[1], &convergeParams.target_fraction, 1)))
                return Usage(argv[0]);
            converge = true;
        } else if (!std::strcmp(argv[i], "--adaptive") && more) {
            const std::vector<std::string> f = Split(argv[++i], ':');
            if (f.size() < 2 || f.size() > 3 || !ParseFloats(f[0], &convergeParams.threshold, 1) ||
                !ParseFloats(f[1], &convergeParams.target_fraction, 1))
                return Usage(argv[0]);
            if (f.size() == 3) adaptiveMargin = (uint32_t)std::atoi(f[2].c_str());
            converge = adaptive = true;
        } else if (!std::strcmp(argv[i], "--firefly")) {
            firefly = true;
            // the optional fields: whatever follows that is not the next option (the positional arguments all come
            // first) has to be four numbers, each read to its end; set_firefly refuses values out of range
            if (more && std::strncmp(argv[i + 1], "--", 2) != 0) {
                const std::vector<std::string> f = Split(argv[++i], ':');
                if (f.size() != 4) return Usage(argv[0]);
                float v[4];
                for (int k = 0; k < 4; ++k) {
                    char* end = nullptr;
                    v[k] = std::strtof(f[k].c_str(), &end);
                    if (f[k].empty() || *end != '\0') return Usage(argv[0]);
                }
                if (!(v[0] >= 0.0f && v[0] <= 64.0f) || v[0] != std::floor(v[0])) return Usage(argv[0]);
                fireflyParams.cascades = (uint32_t)v[0];
                fireflyParams.start = v[1];
                fireflyParams.base = v[2];
                fireflyParams.min_support = v[3];
            }
        } else if (!std::strcmp(argv[i], "--sample-map") && more) {
            sampleMapPath = argv[++i];
        } else if (!std::strcmp(argv[i], "--check-points") && more) {
            const std::vector<std::string> f = Split(argv[++i], ':');
            if (f.size() != 2) return Usage(argv[0]);
            convergeParams.min_images = (uint32_t)std::atoi(f[0].c_str());
            convergeParams.check_interval = (uint32_t)std::atoi(f[1].c_str());
        } else if (!std::strcmp(argv[i], "--noise-map") && more) {
            noiseMapPath = argv[++i];
        } else if (!std::strcmp(argv[i], "--edit") && more) {
            SEdit e;
            if (!ParseEdit(argv[++i], &e)) return Usage(argv[0]);
            edits.push_back(e);
        } else {
            return Usage(argv[0]);
        }
    }
    if (width == 0 || height == 0 || spp == 0 || iterations == 0) return Usage(argv[0]);
    if (batch && !edits.empty()) return Usage(argv[0]);   // (edits belong to the frame loop)
    if (denoise && outputType != DCRT_OUTPUT_PATH_TRACING) return Usage(argv[0]);   // (a view is noise-free)
    if ((noiseMapPath && !converge) || (converge && (!edits.empty() || spp < 2))) return Usage(argv[0]);
    if (converge) {
        batch = true;   // (render_converged sequences the images on the device, as --batch does)
        convergeParams.max_images = spp;
        convergeParams.min_images = std::max(2u, std::min(convergeParams.min_images, spp));
    }

    // CDirectComputeRayTracing::Init: new + Create (LaunchRendererLoop.cpp:58-64)
    CScene scene;
    CMI355XPathTracer tracer(pool ? pool : (batch ? (1u << 24) : (1u << 21)), iterations);
    CRendererLoop loop(&scene, &tracer);
    loop.m_FrameSeedType = seedType;
    if (!scene.m_Handle) return 1;
    if (!tracer.Create()) return 1;
    if (outputType != DCRT_OUTPUT_PATH_TRACING && !tracer.SetOutputType(outputType, iterationThreshold)) return 1;
    if (roulette.enable && !tracer.SetRoulette(roulette)) return 1;   // (on the tracer: kept across uploads and --edit)

    // LoadScene: Reset + LoadFromFile (+ UI "Create -> Point Light", max bounce), then
    // OnSceneLoaded and the small-resolution size
    scene.m_IsFilmDirty = true;
    if (!scene.Reset(width, height) || !scene.LoadFromFile(scenePath)) {
        std::fprintf(stderr, "LoadScene failed: %s\n", dcrt_last_error());
        return 1;
    }
    if (pointLight) {
        const float euler[3] = {0, 0, 0};
        if (!Check(dcrt_scene_add_punctual_light(scene.m_Handle, lightPos, euler, lightColor, 0), "AddPointLight")) return 1;
    }
    if (!Check(dcrt_scene_set_max_bounce(scene.m_Handle, maxBounce), "SetMaxBounce")) return 1;
    if (!loop.AfterSceneEdited()) return 1;
    if (envImportance && !tracer.SetEnvironmentSampling(DCRT_ENV_SAMPLING_IMPORTANCE)) return 1;   // (on the uploaded scene; kept across --edit uploads)
    if (lightPower && !tracer.SetLightSampling(DCRT_LIGHT_SAMPLING_POWER)) return 1;
    if (seedType == CRendererLoop::EFrameSeedType::Fixed) scene.m_FrameSeed = fixedSeed;   // the UI's seed field (ImGui.cpp:157-160)
    // (on the tracer's film, which the upload sized; kept across --edit uploads and the preview frames' resolution changes)
    if (firefly && !Check(dcrt_tracer_set_firefly(tracer.GetTracer(), &fireflyParams), "SetFirefly")) return 1;

    const auto t0 = std::chrono::steady_clock::now();
    uint32_t firstSeed = 0;
    uint64_t previewFrames = 0;
    size_t editsApplied = 0;
    std::vector<uint32_t> seeds;  // frame seed of each full-resolution image, in film order
    uint32_t images = spp;        // images in the film (--converge: as many as it took)
    dcrt_noise_stats noise = {};
    int converged = 0;
    dcrt_adaptive_report adaptiveReport = {};
    if (adaptive) {
        const dcrt_filter_params filter = MakeFilter(scene);
        if (!Check(dcrt_tracer_set_convergence(tracer.GetTracer(), 1), "SetConvergence") ||
            !Check(dcrt_tracer_set_adaptive(tracer.GetTracer(), 1), "SetAdaptive") ||
            !Check(dcrt_tracer_render_adaptive(tracer.GetTracer(), 0, &convergeParams, adaptiveMargin, &filter, &noise, &converged,
                                               &adaptiveReport),
                   "RenderAdaptive"))
            return 1;
        images = noise.images;
        for (uint32_t s = 0; s < images; ++s) seeds.push_back(s);
    } else if (converge) {
        const dcrt_filter_params filter = MakeFilter(scene);
        if (!Check(dcrt_tracer_set_convergence(tracer.GetTracer(), 1), "SetConvergence") ||
            !Check(dcrt_tracer_render_converged(tracer.GetTracer(), 0, &convergeParams, &filter, &noise, &converged), "RenderConverged"))
            return 1;
        images = noise.images;
        for (uint32_t s = 0; s < images; ++s) seeds.push_back(s);
    } else if (batch) {
        const dcrt_filter_params filter = MakeFilter(scene);
        if (!Check(dcrt_tracer_clear_film(tracer.GetTracer()), "ClearFilm") ||
            !Check(dcrt_tracer_render_images(tracer.GetTracer(), 0, spp, &filter), "RenderImages"))
            return 1;
        for (uint32_t s = 0; s < spp; ++s) seeds.push_back(s);
    } else {
        // RenderOneFrame until spp full-resolution images are in the film
        // (with edits: until spp images have completed after the last one)
        uint64_t imagesWanted = spp;
        for (const SEdit& e : edits) imagesWanted += e.m_AfterImages;
        const uint64_t maxFrames = imagesWanted * 100000ull + 1000ull;
        uint32_t imagesSinceEdit = 0;
        // the load's own dirty bits are spent: AfterSceneEdited uploaded everything
        uint32_t spentBits = 0;
        if (!edits.empty() && !Check(dcrt_scene_acquire_dirty(scene.m_Handle, &spentBits), "AcquireDirty")) return 1;
        while (seeds.size() < spp || editsApplied < edits.size()) {
            SRenderContext rc;
            if (!loop.RenderOneFrame(&rc)) return 1;
            if (rc.m_IsSmallResolutionEnabled) {
                ++previewFrames;
                continue;
            }
            // (the seed advances right after the image completes, except under Fixed)
            if (loop.m_LastFrameCompletedImage) {
                seeds.push_back(seedType == CRendererLoop::EFrameSeedType::Fixed ? scene.m_FrameSeed : scene.m_FrameSeed - 1u);
                ++imagesSinceEdit;
            }
            if (editsApplied < edits.size() && imagesSinceEdit >= edits[editsApplied].m_AfterImages) {
                // between two frames, as the UI edits: the next frame finds the dirty flags, restarts
                // the film with a preview and sends only the edited arrays
                if (!ApplyEdit(scene.m_Handle, edits[editsApplied]) || !scene.AcquireEdits()) return 1;
                ++editsApplied;
                imagesSinceEdit = 0;
                seeds.clear();   // (the film restarts: its images are the ones after the edit)
            }
            if (loop.m_FrameIndex > maxFrames) {
                std::fprintf(stderr, "the frame loop did not complete %u images\n", spp);
                return 1;
            }
        }
        firstSeed = seeds.empty() ? 0 : seeds.front();
    }
    if (!Check(dcrt_tracer_synchronize(tracer.GetTracer()), "Synchronize")) return 1;
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const uint32_t W = scene.m_ResolutionWidth, H = scene.m_ResolutionHeight;   // (an XML scene sets its own)
    const size_t n = (size_t)W * H;
    if (filmPath) {
        std::vector<float> film(n * 4);
        if (!Check(dcrt_tracer_read_film(tracer.GetTracer(), film.data()), "ReadFilm") || !WriteFloats(filmPath, film)) return 1;
    }
    if (samplesPath) {
        std::vector<float> pos(n * 2), val(n * 4);
        if (!Check(dcrt_tracer_read_samples(tracer.GetTracer(), pos.data(), val.data()), "ReadSamples") ||
            !WriteFloats(samplesPath, pos, &val))
            return 1;
    }
    // post-processing + "Save Image to File"
    dcrt_postfx_params post;
    if (!Check(dcrt_scene_get_postfx_params(scene.m_Handle, &post), "GetPostFxParams")) return 1;
    std::vector<uint8_t> rgba(n * 4);
    float sumLogLuminance = 0.0f;
    double fireflyRemoved = 0.0;   // the share of the film's summed luminance the resolve took out
    if (firefly) {
        std::vector<float> film(n * 4), kept(n * 4);
        if (!Check(dcrt_tracer_firefly_resolve(tracer.GetTracer()), "FireflyResolve") ||
            !Check(dcrt_tracer_read_film(tracer.GetTracer(), film.data()), "ReadFilm") ||
            !Check(dcrt_tracer_read_firefly(tracer.GetTracer(), kept.data()), "ReadFirefly"))
            return 1;
        double before = 0.0, after = 0.0;
        for (size_t p = 0; p < n; ++p) {
            const float* f = &film[4 * p];
            const float* k = &kept[4 * p];
            if (f[3] > 0.0f) before += std::fmax(0.0, (0.299 * f[0] + 0.587 * f[1] + 0.114 * f[2]) / f[3]);
            after += std::fmax(0.0, 0.299 * k[0] + 0.587 * k[1] + 0.114 * k[2]);
        }
        fireflyRemoved = before > 0.0 ? 1.0 - after / before : 0.0;
    }
    if (denoise) {
        // the guides of the film's own images: the same seeds, so the same sub-pixel positions
        // (a fixed seed repeats one image: its guides are every image's)
        bool consecutive = !seeds.empty(), equal = !seeds.empty();
        for (size_t i = 0; i < seeds.size(); ++i) {
            consecutive = consecutive && seeds[i] == seeds[0] + (uint32_t)i;
            equal = equal && seeds[i] == seeds[0];
        }
        if (!consecutive && !equal) {
            std::fprintf(stderr, "--denoise: the film's frame seeds are not consecutive (use sample-count seeds or --batch)\n");
            return 1;
        }
        dcrt_denoise_params dn;
        if (!Check(dcrt_denoise_default_params(&dn), "DenoiseDefaultParams") ||
            !Check(dcrt_tracer_render_guides(tracer.GetTracer(), seeds[0], consecutive ? (uint32_t)seeds.size() : 1u), "RenderGuides") ||
            // (with --firefly the re-weighted image is the colour input)
            !Check(firefly ? dcrt_tracer_denoise_firefly(tracer.GetTracer(), &dn) : dcrt_tracer_denoise(tracer.GetTracer(), &dn), "Denoise"))
            return 1;
        if (!Check(dcrt_tracer_resolve_denoised(tracer.GetTracer(), &post, rgba.data(), &sumLogLuminance), "ResolveDenoised")) return 1;
    } else if (firefly) {
        if (!Check(dcrt_tracer_resolve_firefly(tracer.GetTracer(), &post, rgba.data(), &sumLogLuminance), "ResolveFirefly")) return 1;
    } else if (!Check(dcrt_tracer_resolve_image(tracer.GetTracer(), &post, rgba.data(), &sumLogLuminance), "ResolveImage")) {
        return 1;
    }
    if (!Check(dcrt_write_bmp(outPath, W, H, rgba.data()), "WriteBmp")) return 1;
    if (noiseMapPath) {
        std::vector<float> e(n);
        if (!Check(dcrt_tracer_read_noise_maps(tracer.GetTracer(), e.data(), nullptr), "ReadNoiseMaps")) return 1;
        std::vector<uint8_t> grey(n * 4);
        for (size_t p = 0; p < n; ++p) {
            const float v = std::fmin(e[p] / convergeParams.threshold, 1.0f);
            const uint8_t code = v != v ? 255 : (uint8_t)(int)(v * 255.0f + 0.5f);
            grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = code;
            grey[4 * p + 3] = 255;
        }
        if (!Check(dcrt_write_bmp(noiseMapPath, W, H, grey.data()), "WriteBmp (noise map)")) return 1;
    }
    if (sampleMapPath) {
        std::vector<float> film(n * 4);
        if (!Check(dcrt_tracer_read_film(tracer.GetTracer(), film.data()), "ReadFilm")) return 1;
        float top = 0.0f;
        for (size_t p = 0; p < n; ++p) top = std::fmax(top, film[4 * p + 3]);
        std::vector<uint8_t> grey(n * 4);
        for (size_t p = 0; p < n; ++p) {
            const float v = top > 0.0f ? std::fmin(std::fmax(film[4 * p + 3], 0.0f) / top, 1.0f) : 0.0f;
            grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = (uint8_t)(int)(v * 255.0f + 0.5f);
            grey[4 * p + 3] = 255;
        }
        if (!Check(dcrt_write_bmp(sampleMapPath, W, H, grey.data()), "WriteBmp (sample map)")) return 1;
    }
    dcrt_ray_stats stats;
    if (!Check(dcrt_tracer_counters(tracer.GetTracer(), &stats), "Counters")) return 1;
    const double rays = (double)(stats.extension_rays + stats.shadow_rays);
    std::string seedList;
    for (size_t i = 0; i < seeds.size(); ++i) seedList += (i ? "," : "") + std::to_string(seeds[i]);
    std::string editReport;   // (only with --edit: the line is otherwise what it always was)
    if (!edits.empty()) {
        dcrt_upload_stats up;
        if (!tracer.GetUploadStats(&up)) return 1;
        char buf[512];
        std::snprintf(buf, sizeof(buf),
                      ", \"edits_applied\": %zu, \"upload_stats\": {\"scene_uploads\": %llu, \"material_updates\": %llu, "
                      "\"light_updates\": %llu, \"instance_flag_updates\": %llu, \"geometry_bytes\": %llu, \"shading_bytes\": %llu, "
                      "\"graph_invalidations\": %llu}",
                      editsApplied, (unsigned long long)up.scene_uploads, (unsigned long long)up.material_updates,
                      (unsigned long long)up.light_updates, (unsigned long long)up.instance_flag_updates,
                      (unsigned long long)up.geometry_bytes, (unsigned long long)up.shading_bytes,
                      (unsigned long long)up.graph_invalidations);
        editReport = buf;
    }
    if (converge) {   // (only with --converge)
        char buf[512];
        std::snprintf(buf, sizeof(buf),
                      ", \"converged\": %d, \"noise\": {\"images\": %u, \"valid_pixels\": %u, \"converged_pixels\": %u, "
                      "\"mean_error\": %.9g, \"max_error\": %.9g, \"max_tile_error\": %.9g}",
                      converged, noise.images, noise.valid_pixels, noise.converged_pixels, (double)noise.mean_error, (double)noise.max_error,
                      (double)noise.max_tile_error);
        editReport += buf;
    }
    if (adaptive) {   // (only with --adaptive)
        char buf[256];
        std::snprintf(buf, sizeof(buf),
                      ", \"adaptive\": {\"images\": %u, \"check_points\": %u, \"pixel_samples\": %llu, \"active_blocks\": %u, "
                      "\"total_blocks\": %u}",
                      adaptiveReport.images, adaptiveReport.check_points, (unsigned long long)adaptiveReport.pixel_samples,
                      adaptiveReport.active_blocks, adaptiveReport.total_blocks);
        editReport += buf;
    }
    if (firefly) {   // (only with --firefly)
        char buf[256];
        std::snprintf(buf, sizeof(buf), ", \"firefly\": {\"cascades\": %u, \"start\": %.9g, \"base\": %.9g, \"min_support\": %.9g, \"removed\": %.6g}",
                      fireflyParams.cascades, (double)fireflyParams.start, (double)fireflyParams.base, (double)fireflyParams.min_support,
                      fireflyRemoved);
        editReport += buf;
    }
    std::printf("{\"images\": %u, \"seconds\": %.4f, \"ms_per_spp\": %.3f, \"mrays_per_s\": %.1f, \"extension_rays\": %llu, "
                "\"shadow_rays\": %llu, \"mode\": \"%s\", \"frames\": %llu, \"preview_frames\": %llu, \"first_seed\": %u, "
                "\"seeds\": [%s]%s}\n",
                images, seconds, seconds * 1e3 / images, rays / seconds / 1e6, (unsigned long long)stats.extension_rays,
                (unsigned long long)stats.shadow_rays, adaptive ? "render_adaptive" : converge ? "render_converged" : batch ? "render_images" : "frame_loop", (unsigned long long)loop.m_FrameIndex,
                (unsigned long long)previewFrames, firstSeed, seedList.c_str(), editReport.c_str());
    return 0;
}
