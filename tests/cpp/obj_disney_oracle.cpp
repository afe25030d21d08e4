// tests/cpp/obj_disney_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of rt_wavefront_load_flags: tests/cpp/scatter_oracle.cpp
// (the top of the include chain: the oracle's C ABI with the Disney and Portal
// materials and the radiance and scatter drivers, so one library holds every
// extension) plus
//   orc_wavefront_load_flags -- Wavefont::new in full: load_materials and
//     load_object (shapes/obj.rs:137-345) restated from the reference's lines
//     (cited) with the Disney arm of obj.rs:279-292, on the oracle's own
//     load_obj_file (tobj restated, oracle/rt_oracle_obj.cpp),
//     RemappedMaterial, orc_load_image and orc::Disney -- not from
//     raytracer-2025_amd/csrc/rt_obj.cpp.  Without RT_OBJ_DISNEY it is
//     orc_wavefront_load, refusal included.
// Built at test time by tests/obj_disney_query.py (g++ -ffp-contract=off
// -DORC_CRMATH, with oracle/rt_oracle.cpp and oracle/rt_oracle_obj.cpp).
#include "scatter_oracle.cpp"

namespace {

// material.unknown_param.get(key).and_then(|s| s.parse::<f64>().ok()) (obj.rs:230-259): the whole value parses, or None
std::optional<double> parse_f64(const std::string& v) {
    if (v.empty()) return std::nullopt;
    char* end = nullptr;
    const double x = std::strtod(v.c_str(), &end);
    if (*end != 0) return std::nullopt;
    return x;
}
double unknown_or(const ObjMaterial& m, const char* key, double fallback) {  // .unwrap_or(fallback)
    const auto it = m.unknown_param.find(key);
    if (it == m.unknown_param.end()) return fallback;
    return parse_f64(it->second).value_or(fallback);
}
// .split_whitespace().filter_map(|s| s.parse::<f64>().ok()).collect() (obj.rs:262-265, 296-299)
std::vector<double> numbers_of(const std::string& v) {
    std::vector<double> out;
    std::istringstream is(v);
    std::string word;
    while (is >> word)
        if (const auto x = parse_f64(word)) out.push_back(*x);
    return out;
}

struct Refused {  // what the C entry point answers instead of a Wavefont
    int32_t code;
    std::string what;
};

// ImageTexture::new(prefix/file) (texture.rs:82-88) and new_raw_image (90-97): a file that cannot be read is 0 x 0, cyan
std::shared_ptr<ImageTexture> image_texture(const std::string& prefix, const std::string& file, bool raw) {
    auto t = std::make_shared<ImageTexture>();
    uint32_t w = 0, h = 0;
    if (!orc_load_image(prefix + "/" + file, raw, w, h, t->rgba))
        throw Refused{RT_EUNSUPPORTED, prefix + "/" + file + ": not a PNG"};
    t->w = (int)w;
    t->h = (int)h;
    t->linear_interp = raw;
    return t;
}

// load_materials (obj.rs:212-345)
void load_materials(std::vector<std::shared_ptr<Material>>& mats, std::vector<std::shared_ptr<Texture>>& normals,
                    const std::vector<ObjMaterial>& materials, const std::string& prefix, bool vanilla_material) {
    const auto transparent_mat = std::make_shared<Transparent>();  // :219
    for (const ObjMaterial& material : materials) {               // :221
        std::shared_ptr<Texture> base_color;                       // :222-229
        if (!material.diffuse_texture.empty())
            base_color = image_texture(prefix, material.diffuse_texture, false);
        else if (material.has_diffuse)
            base_color = std::make_shared<SolidColor>(material.diffuse);
        else
            throw Panic("The material should at least have one diffuse!");
        const double roughness = unknown_or(material, "Pr", 0.5);        // :230-234
        const double anisotropic = unknown_or(material, "aniso", 0.0);   // :235-239
        const double sheen = unknown_or(material, "Ps", 0.0);            // :240-244
        const double metallic = unknown_or(material, "Pm", 0.0);         // :245-249
        const double clearcoat = unknown_or(material, "Pc", 0.0);        // :250-254
        const double clearcoat_gloss = unknown_or(material, "Pcr", 0.0); // :255-259
        const double ior = material.has_optical_density ? material.optical_density : 1.45;  // :260
        double spec_trans = 0.0;                                         // :261-269
        if (const auto tf = material.unknown_param.find("Tf"); tf != material.unknown_param.end()) {
            const std::vector<double> spec_trans_vals = numbers_of(tf->second);
            double sum = 0.0;
            for (double x : spec_trans_vals) sum += x;
            spec_trans = sum / (double)spec_trans_vals.size();  // no number: 0 / 0
        }

        std::shared_ptr<Material> mat;  // :271-293
        if (vanilla_material && metallic == 1.0) {
            mat = std::make_shared<Metal>(base_color->value(0.0, 0.0, Vec3(0, 0, 0)), roughness);
        } else if (vanilla_material && spec_trans == 1.0) {
            mat = std::make_shared<Dielectric>(base_color, ior);
        } else {
            orc::DisneyParameters p;  // ..Default::default()
            p.roughness = roughness;
            p.anisotropic = anisotropic;
            p.sheen = sheen;
            p.clearcoat = clearcoat;
            p.clearcoat_gloss = clearcoat_gloss;
            p.metallic = metallic;
            p.ior = ior;
            p.spec_trans = spec_trans;
            // rt_wavefront_load_flags' contract: a parameter that is not finite renders NaNs, and is refused by name
            const std::pair<const char*, double> keys[] = {{"Pr", roughness}, {"aniso", anisotropic}, {"Ps", sheen},
                                                           {"Pm", metallic},  {"Pc", clearcoat},      {"Pcr", clearcoat_gloss},
                                                           {"Ni", ior},       {"Tf", spec_trans}};
            for (const auto& k : keys)
                if (!std::isfinite(k.second))
                    throw Refused{RT_EUNSUPPORTED, "material '" + material.name + "': the Disney parameter of `" + k.first +
                                                       "` is not finite"};
            mat = std::make_shared<orc::Disney>(base_color, p);
        }

        if (const auto emit = material.unknown_param.find("Ke"); emit != material.unknown_param.end()) {  // :295-304
            const std::vector<double> emit_vals = numbers_of(emit->second);
            if (emit_vals.size() == 3)
                mat = std::make_shared<DiffuseLight>(
                    std::make_shared<SolidColor>(Vec3(emit_vals[0], emit_vals[1], emit_vals[2])), mat);
        }
        if (const auto emit = material.unknown_param.find("map_Ke"); emit != material.unknown_param.end())  // :306-310
            mat = std::make_shared<DiffuseLight>(image_texture(prefix, emit->second, false), mat);
        if (!material.dissolve_texture.empty())  // :312-319
            mat = std::make_shared<Mix>(transparent_mat, mat, image_texture(prefix, material.dissolve_texture, false));
        if (material.has_dissolve && material.dissolve < 1.0)  // :320-324
            mat = std::make_shared<Mix>(transparent_mat, mat, material.dissolve);
        mats.push_back(mat);  // :326

        if (!material.normal_texture.empty()) {  // :328-343: "file" or "-bm 1.000000 file"
            std::string file = material.normal_texture;
            if (file.rfind("-bm", 0) == 0) {
                std::istringstream parts(file.substr(3));
                std::string part, last;
                while (parts >> part) last = part;
                if (!last.empty()) file = last;
            }
            normals.push_back(image_texture(prefix, file, true));
        } else {
            normals.push_back(nullptr);
        }
    }
}

// Wavefont::get_three_values / get_two_values (obj.rs:106-115): slice indexing, a panic past the end
Vec3 get_three_values(const std::vector<double>& a, size_t i) {
    if (i * 3 + 2 >= a.size()) throw Panic("index out of bounds (obj.rs:107-110)");
    return Vec3(a[i * 3], a[i * 3 + 1], a[i * 3 + 2]);
}
Vec3 get_two_values(const std::vector<double>& a, size_t i) {
    if (i * 2 + 1 >= a.size()) throw Panic("index out of bounds (obj.rs:112-115)");
    return Vec3(a[i * 2], a[i * 2 + 1], 0.0);
}

// load_object (obj.rs:137-194) with uv_local_to_world (196-210)
void load_object(const std::vector<std::shared_ptr<Material>>& mats, Hittables& obs, const ObjModel& object,
                 const std::shared_ptr<Texture>& normal_texture) {
    const auto empty_material = std::make_shared<EmptyMaterial>();  // :144
    std::vector<HittablePtr> v;                                     // :146
    for (size_t k = 0; k + 2 < object.indices.size(); k += 3) {     // :147
        const uint32_t* indices = &object.indices[k];
        const Vec3 p1 = get_three_values(object.positions, indices[0]);  // :148-150
        const Vec3 p2 = get_three_values(object.positions, indices[1]);
        const Vec3 p3 = get_three_values(object.positions, indices[2]);
        const Vec3 tex_p1 = get_two_values(object.texcoords, indices[0]);  // :152-154
        const Vec3 tex_p2 = get_two_values(object.texcoords, indices[1]);
        const Vec3 tex_p3 = get_two_values(object.texcoords, indices[2]);
        const Vec3 n_p1 = get_three_values(object.normals, indices[0]);  // :156-158
        const Vec3 n_p2 = get_three_values(object.normals, indices[1]);
        const Vec3 n_p3 = get_three_values(object.normals, indices[2]);
        auto rm = std::make_shared<RemappedMaterial>();  // :174-183
        rm->material = object.material_id >= 0 ? mats.at((size_t)object.material_id) : empty_material;  // :160-164
        const Vec3 tex_u = tex_p2 - tex_p1, tex_v = tex_p3 - tex_p1;  // :166-167
        const Vec3 world_u = p2 - p1, world_v = p3 - p1;              // :169-170
        // :202-208
        const double ua = tex_v.e[1] / (-tex_u.e[1] * tex_v.e[0] + tex_u.e[0] * tex_v.e[1]);
        const double ub = tex_u.e[1] / (tex_u.e[1] * tex_v.e[0] - tex_u.e[0] * tex_v.e[1]);
        const double va = tex_v.e[0] / (tex_u.e[1] * tex_v.e[0] - tex_u.e[0] * tex_v.e[1]);
        const double vb = tex_u.e[0] / (-tex_u.e[1] * tex_v.e[0] + tex_u.e[0] * tex_v.e[1]);
        rm->u_vec = from_vec3(world_u * ua + world_v * ub);
        rm->v_vec = from_vec3(world_u * va + world_v * vb);
        rm->tex_ori = tex_p1;
        rm->tex_u = tex_u;
        rm->tex_v = tex_v;
        rm->normal[0] = n_p1;
        rm->normal[1] = n_p2;
        rm->normal[2] = n_p3;
        rm->normal_tex = normal_texture;
        if (auto triangle = make_triangle(p1, world_u, world_v, rm)) v.push_back(std::move(triangle));  // :185-187
    }
    if (!v.empty()) obs.add(BVH::from_vec(std::move(v)));  // :189-193
}

}  // namespace

extern "C" int32_t orc_wavefront_load_flags(rt_scene* s, const char* obj_path, uint32_t flags) {
    if (flags & ~(RT_OBJ_VANILLA | RT_OBJ_DISNEY)) return fail(RT_EINVAL, "unknown rt_wavefront_load_flags flags");
    if (!(flags & RT_OBJ_DISNEY)) return orc_wavefront_load(s, obj_path, (flags & RT_OBJ_VANILLA) ? 1 : 0);
    if (!s || !obj_path) return fail(RT_EINVAL, "null");
    GUARD_BEGIN
    // Wavefont::new (obj.rs:117-134); file_path = prefix + "/" + file_name, given whole here
    const std::string path(obj_path);
    const size_t slash = path.rfind('/');
    const std::string prefix = slash == std::string::npos ? "." : path.substr(0, slash);
    const ObjFile f = load_obj_file(obj_path);  // :119 (.ok()?: the throw is RT_EINVAL)
    std::vector<std::shared_ptr<Material>> mats;
    std::vector<std::shared_ptr<Texture>> normals;
    try {
        if (f.materials_ok) load_materials(mats, normals, f.materials, prefix, (flags & RT_OBJ_VANILLA) != 0);  // :123-125
    } catch (const Refused& r) {
        return fail(r.code, r.what);
    }
    auto obs = std::make_unique<Hittables>();  // :127
    for (size_t i = 0; i < f.models.size() && i < normals.size(); ++i)  // objects.iter().zip(normals.iter()), :129
        load_object(mats, *obs, f.models[i], normals[i]);
    return s->add_obj(std::move(obs));
    GUARD_END
}
